"""Host-side Python mirror of the reference's call shapes for the hot path, over the C ABI.

Names follow the reference so that the parity tests read like its call sites:

  RandomForest.read / classLogPosterior / multiClassLogPosterior   (libforest classifiers.h:274-344)
  FeatureExtractor.extract                                         (include/feature_extractor.h:41)
  DenseCRF(N, C).setUnaryEnergy / addPairwiseEnergy / inference / map  (densecrf.h:36-121)
    + learned models: Potts / Diagonal / MatrixCompatibility, kernel types, normalisations, logistic unary and the
      parameter vectors of densecrf.cpp:294-360 (labelcompatibility.h, pairwise.h:32-42, unary.h)
  Segmenter.processFrames                                          (src/segmenter.cpp:323-443; with
    external_semantics the other provider, processFramesFromQueueExternal, :445-514)
  RgbLabelConversion.rgbToLabel / labelToRgb / getLabelName / ...  (include/rgb_label_conversion.h)
  Evaluator: the confusion matrix and scores of src/test.cpp:182-228 (test_multi.cpp:222-268)

All compute happens in librvseg.so (HIP, gfx950).  Nothing here falls back to the CPU.
"""
import ctypes as C

import numpy as np

from . import _capi as capi


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """Owns one rvseg_ctx (one per thread and device, as include/rvseg.h requires)."""

    def __init__(self, schedule=None, **params):
        """params: fields of rvseg_params; schedule: dict of rvseg_schedule fields (launch-schedule overrides for
        tests, profiling and tuning -- the library reads no environment variables)."""
        self.params = capi.default_params(**params)
        h = C.c_void_p()
        st = capi.lib().rvseg_create(C.byref(self.params), C.byref(h))
        if st != capi.OK:
            raise capi.RvsegError(st, capi.lib().rvseg_last_error(None).decode("utf-8", "replace"))
        self.h = h
        self.L = capi.lib()
        if schedule:
            self.set_schedule(**schedule)

    def set_schedule(self, **kw):
        """rvseg_set_schedule: the defaults with the given rvseg_schedule fields replaced."""
        sc = capi.RvsegSchedule()
        self.L.rvseg_schedule_default(C.byref(sc))
        known = {f[0] for f in capi.RvsegSchedule._fields_}
        for k, v in kw.items():
            if k not in known:
                raise TypeError("unknown rvseg_schedule field %r" % k)
            setattr(sc, k, int(v))
        capi.check(self.h, self.L.rvseg_set_schedule(self.h, C.byref(sc)))

    def last_schedule(self):
        """rvseg_last_schedule as a dict; `splat` as a name ("list-major" / "resident").  `vertices` and
        `planner_fallback` are -1 until poll_status(wait=True) (or a host entry point) has returned."""
        info = capi.RvsegScheduleInfo()
        capi.check(self.h, self.L.rvseg_last_schedule(self.h, C.byref(info)))
        d = {f[0]: getattr(info, f[0]) for f in capi.RvsegScheduleInfo._fields_}
        d["splat"] = capi.SPLAT_NAMES.get(d["splat"], str(d["splat"]))
        return d

    def close(self):
        if getattr(self, "h", None):
            self.L.rvseg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- forest ------------------------------------------------------------------------------
    @property
    def feature_length(self):
        return self.L.rvseg_feature_length(self.h)

    def forest_load(self, src):
        if isinstance(src, (bytes, bytearray, memoryview)):
            buf = bytes(src)
            capi.check(self.h, self.L.rvseg_forest_load_mem(self.h, buf, len(buf)))
        else:
            capi.check(self.h, self.L.rvseg_forest_load(self.h, str(src).encode()))

    def forest_write(self, path=None):
        """RandomForest::write (classifier.cpp:210-220): to `path`, or returns the bytes."""
        if path is not None:
            capi.check(self.h, self.L.rvseg_forest_write(self.h, str(path).encode()))
            return None
        size = C.c_size_t()
        capi.check(self.h, self.L.rvseg_forest_write_mem(self.h, None, 0, C.byref(size)))
        buf = C.create_string_buffer(size.value)
        capi.check(self.h, self.L.rvseg_forest_write_mem(self.h, buf, size.value, C.byref(size)))
        return buf.raw[:size.value]

    def forest_train(self, X, labels, class_counts, class_prior=None, **train_params):
        """rvseg_forest_train: X (P, D) float32, labels (P, L) int32 class indices.  Returns the forest.dat bytes.
        train_params: fields of rvseg_train_params (num_trees, max_depth, min_split_examples, ...).
        class_prior: None (the unweighted split objective), "inverse_frequency" (libforest's useClassFrequency) or one
        weight per class -- rvseg_forest_train_prior, one layer only."""
        X = np.ascontiguousarray(X, np.float32)
        labels = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(X.shape[0], -1))
        P, D = X.shape
        L = labels.shape[1]
        assert len(class_counts) == L
        if class_prior is not None and L != 1:
            raise ValueError("class_prior: the class-weighted objective trains single-layer forests only")
        tp = self._train_params(train_params)
        cc = (C.c_int32 * L)(*class_counts)
        size = C.c_size_t()
        # trains once (the model stays on the context), then fetches it into a buffer of the right size
        if class_prior is None:
            capi.check(self.h, self.L.rvseg_forest_train(self.h, _ptr(X), P, D, _ptr(labels), L, cc, C.byref(tp), None, 0, C.byref(size)))
        else:
            prior = self._class_prior(class_prior, class_counts[0])
            capi.check(self.h, self.L.rvseg_forest_train_prior(self.h, _ptr(X), P, D, _ptr(labels), class_counts[0], C.byref(tp),
                                                               C.byref(prior), None, 0, C.byref(size)))
        return self._trained_model(size.value)

    @staticmethod
    def _class_prior(class_prior, n_classes):
        """rvseg_class_prior from "inverse_frequency" or a sequence of n_classes weights."""
        prior = capi.RvsegClassPrior()
        if isinstance(class_prior, str):
            if class_prior != "inverse_frequency":
                raise ValueError("class_prior: None, 'inverse_frequency' or one weight per class, not %r" % class_prior)
            prior.mode = capi.PRIOR_INVERSE_FREQUENCY
            return prior
        w = np.asarray(class_prior, np.float32).reshape(-1)
        if w.shape[0] != n_classes or n_classes > 16:
            raise ValueError("class_prior: %d weights for %d classes (at most 16)" % (w.shape[0], n_classes))
        prior.mode = capi.PRIOR_GIVEN
        for c in range(n_classes):
            prior.weights[c] = w[c]
        return prior

    def _train_params(self, train_params):
        tp = capi.RvsegTrainParams()
        self.L.rvseg_train_params_default(C.byref(tp))
        known = {f[0] for f in capi.RvsegTrainParams._fields_}
        for k, v in train_params.items():
            if k not in known:
                raise TypeError("unknown rvseg_train_params field %r" % k)
            setattr(tp, k, v)
        return tp

    def _trained_model(self, size):
        buf = C.create_string_buffer(size)
        got = C.c_size_t()
        capi.check(self.h, self.L.rvseg_forest_train_result(self.h, buf, size, C.byref(got)))
        return buf.raw[:got.value]

    # ---- boosted forest (libf::BoostedRandomForest / BoostedRandomForestLearner) ---------------
    def boosted_load(self, src, order=capi.BOOSTED_WEIGHT_FIRST):
        """BoostedRandomForest::read (classifier.cpp:264-280) of a stream in `order`: BOOSTED_WEIGHT_FIRST is what the
        reference's write produces, BOOSTED_TREE_FIRST what its read accepts.  forest_eval then returns the vote sums."""
        if isinstance(src, (bytes, bytearray, memoryview)):
            buf = bytes(src)
            capi.check(self.h, self.L.rvseg_boosted_load_mem(self.h, buf, len(buf), order))
        else:
            capi.check(self.h, self.L.rvseg_boosted_load(self.h, str(src).encode(), order))

    def boosted_write(self, path=None, order=capi.BOOSTED_AS_LOADED):
        """BoostedRandomForest::write (classifier.cpp:250-262): to `path`, or returns the bytes.  The default order is the
        one the model was read in."""
        if path is not None:
            capi.check(self.h, self.L.rvseg_boosted_write(self.h, str(path).encode(), order))
            return None
        size = C.c_size_t()
        capi.check(self.h, self.L.rvseg_boosted_write_mem(self.h, order, None, 0, C.byref(size)))
        buf = C.create_string_buffer(size.value)
        capi.check(self.h, self.L.rvseg_boosted_write_mem(self.h, order, buf, size.value, C.byref(size)))
        return buf.raw[:size.value]

    def boosted_weights(self):
        """BoostedRandomForest::getWeights: float32 (T,), as the stream holds them."""
        n = C.c_int32()
        capi.check(self.h, self.L.rvseg_boosted_weights(self.h, None, 0, C.byref(n), None))
        out = np.empty(n.value, np.float32)
        capi.check(self.h, self.L.rvseg_boosted_weights(self.h, _ptr(out), n.value, C.byref(n), None))
        return out

    def boosted_train(self, X, labels, n_classes, class_prior=None, **train_params):
        """rvseg_boosted_train: X (P, D) float32, labels (P,) int32 class indices of n_classes classes; num_trees is the
        number of boosting rounds.  Returns dict(model = the BOOSTED_WEIGHT_FIRST stream, rounds = trees kept, errors,
        alphas = float32 (num_trees,), NaN where a round did not run or kept no tree).  class_prior: as forest_train's
        (rvseg_boosted_train_prior)."""
        X = np.ascontiguousarray(X, np.float32)
        labels = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(-1))
        P, D = X.shape
        assert labels.shape == (P,)
        tp = self._train_params(train_params)
        errors = np.empty(max(tp.num_trees, 1), np.float32)
        alphas = np.empty(max(tp.num_trees, 1), np.float32)
        size, rounds = C.c_size_t(), C.c_int32()
        if class_prior is None:
            capi.check(self.h, self.L.rvseg_boosted_train(self.h, _ptr(X), P, D, _ptr(labels), n_classes, C.byref(tp), None, 0, C.byref(size),
                                                          _ptr(errors), _ptr(alphas), C.byref(rounds)))
        else:
            prior = self._class_prior(class_prior, n_classes)
            capi.check(self.h, self.L.rvseg_boosted_train_prior(self.h, _ptr(X), P, D, _ptr(labels), n_classes, C.byref(tp), C.byref(prior),
                                                                None, 0, C.byref(size), _ptr(errors), _ptr(alphas), C.byref(rounds)))
        # trained once (the model stays on the context, apart from a loaded one), then fetched into a buffer of the right size
        buf = C.create_string_buffer(size.value)
        capi.check(self.h, self.L.rvseg_boosted_train_result(self.h, capi.BOOSTED_WEIGHT_FIRST, buf, size.value, C.byref(size)))
        return {"model": buf.raw[:size.value], "rounds": rounds.value,
                "errors": errors[:tp.num_trees], "alphas": alphas[:tp.num_trees]}

    def boosted_resample(self, weights, miss=None, exp_alpha=1.0, key=0):
        """rvseg_boosted_resample: one boosting round's weight kernels on caller-supplied weights (N,) >= 0 and miss flags
        (N,) or None.  Returns dict(error, weights, cumsum, idx)."""
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        N = w.shape[0]
        m = None if miss is None else np.ascontiguousarray(np.asarray(miss).reshape(-1) != 0, np.uint8)
        assert m is None or m.shape == (N,)
        err = C.c_float()
        wo, cs, idx = np.empty(N, np.float32), np.empty(N, np.float32), np.empty(N, np.int32)
        capi.check(self.h, self.L.rvseg_boosted_resample(self.h, _ptr(w), _ptr(m) if m is not None else None, N, float(exp_alpha),
                                                         int(key), C.byref(err), _ptr(wo), _ptr(cs), _ptr(idx)))
        return {"error": np.float32(err.value), "weights": wo, "cumsum": cs, "idx": idx}

    def forest_train_frames(self, rgb, depth, calib, labels, class_counts, augment=False, **train_params):
        """rvseg_forest_train_frames: rgb (n, H, W, 3) uint8, depth (n, H, W) uint16, labels (n, L, H, W) int8 (< 0 =
        unlabelled).  Returns (forest.dat bytes, number of training points)."""
        p = self.params
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        labels = np.ascontiguousarray(labels, np.int8)
        n = rgb.shape[0]
        L = labels.shape[1]
        assert rgb.shape == (n, p.height, p.width, 3) and depth.shape == (n, p.height, p.width)
        assert labels.shape == (n, L, p.height, p.width) and len(class_counts) == L
        calib = np.ascontiguousarray(np.broadcast_to(np.asarray(calib, np.float32).reshape(-1, 21), (n, 21)))
        tp = self._train_params(train_params)
        cc = (C.c_int32 * L)(*class_counts)
        size = C.c_size_t()
        n_ex = C.c_int32()
        capi.check(self.h, self.L.rvseg_forest_train_frames(self.h, n, _ptr(rgb), _ptr(depth), _ptr(calib), _ptr(labels), L, cc,
                                                            1 if augment else 0, C.byref(tp), None, 0, C.byref(size), C.byref(n_ex)))
        return self._trained_model(size.value), n_ex.value

    def poll_status(self, wait=True):
        """Status of the asynchronous part of the last segment_frames_device call: capi.OK,
        capi.NOT_READY (only with wait=False) or raises RvsegError(ERR_CAPACITY)."""
        st = self.L.rvseg_poll_status(self.h, 1 if wait else 0)
        if st == capi.NOT_READY:
            return st
        capi.check(self.h, st)
        return st

    def forest_info(self):
        nt, nn, md, nl = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        cc = (C.c_int32 * capi.RVSEG_MAX_LAYERS)()
        capi.check(self.h, self.L.rvseg_forest_info(self.h, C.byref(nt), C.byref(nn), C.byref(md), C.byref(nl), C.byref(cc)))
        return {"n_trees": nt.value, "n_nodes": nn.value, "max_depth": md.value,
                "class_counts": [cc[i] for i in range(nl.value)]}

    def forest_eval(self, X):
        X = np.ascontiguousarray(X, np.float32)
        P, D = X.shape
        S = sum(self.forest_info()["class_counts"])
        out = np.empty((P, S), np.float32)
        capi.check(self.h, self.L.rvseg_forest_eval(self.h, _ptr(X), P, D, _ptr(out)))
        return out

    # ---- forest tools (libforest tools.h; updateHistograms) --------------------------------------
    def forest_classify(self, X, layer=0):
        """rvseg_forest_classify: Classifier::classify on every row of X for the loaded model -> int32 (P,)."""
        X = np.ascontiguousarray(X, np.float32)
        P, D = X.shape
        out = np.empty(P, np.int32)
        capi.check(self.h, self.L.rvseg_forest_classify(self.h, _ptr(X), P, D, layer, _ptr(out)))
        return out

    def forest_classify_trees(self, X, layer=0):
        """rvseg_forest_classify_trees: every tree's own vote -> uint8 (T, P)."""
        X = np.ascontiguousarray(X, np.float32)
        P, D = X.shape
        out = np.empty((self.forest_info()["n_trees"], P), np.uint8)
        capi.check(self.h, self.L.rvseg_forest_classify_trees(self.h, _ptr(X), P, D, layer, _ptr(out)))
        return out

    def forest_measure(self, X, labels=None, layer=0, want=("pred", "confusion", "agree")):
        """rvseg_forest_measure in one pass: dict(pred int32 (P,), confusion uint64 (C, C) [true][predicted], agree uint64
        (T, T)).  Only the outputs named in `want` are computed; the others, and the confusion without labels, are None."""
        X = np.ascontiguousarray(X, np.float32)
        P, D = X.shape
        info = self.forest_info()
        T, Cn = info["n_trees"], (info["class_counts"][layer] if 0 <= layer < len(info["class_counts"]) else 1)
        lab = None if labels is None else np.ascontiguousarray(np.asarray(labels, np.int32).reshape(-1))
        assert lab is None or lab.shape == (P,)
        pred = np.empty(P, np.int32) if "pred" in want else None
        agree = np.empty((T, T), np.uint64) if "agree" in want else None
        conf = np.empty((Cn, Cn), np.uint64) if "confusion" in want and lab is not None else None
        capi.check(self.h, self.L.rvseg_forest_measure(self.h, _ptr(X), P, D, _ptr(lab), layer, _ptr(pred), _ptr(conf), _ptr(agree)))
        return {"pred": pred, "confusion": conf, "agree": agree}

    def forest_refit(self, X, labels, class_counts, smoothing=1.0, return_counts=False):
        """rvseg_forest_refit: the loaded forest with its leaves re-estimated from (X, labels (P, L)).  Returns the
        forest.dat bytes, or (bytes, counts uint32 (n_nodes, sumC)) with return_counts.  The loaded model stays."""
        X = np.ascontiguousarray(X, np.float32)
        labels = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(X.shape[0], -1))
        P, D = X.shape
        L = labels.shape[1]
        assert len(class_counts) == L
        cc = (C.c_int32 * L)(*class_counts)
        size = C.c_size_t()
        capi.check(self.h, self.L.rvseg_forest_refit(self.h, _ptr(X), P, D, _ptr(labels), L, cc, smoothing, None, 0, C.byref(size), None))
        buf = C.create_string_buffer(size.value)
        counts = np.empty((self.forest_info()["n_nodes"], sum(class_counts)), np.uint32) if return_counts else None
        capi.check(self.h, self.L.rvseg_forest_refit(self.h, _ptr(X), P, D, _ptr(labels), L, cc, smoothing, buf, size.value, C.byref(size),
                                                     _ptr(counts)))
        return (buf.raw[:size.value], counts) if return_counts else buf.raw[:size.value]

    # ---- forest pruning (libforest todos.txt: RandomForestPrune over mcmc.h's simulated annealing) ----
    def _prune_state(self, state):
        """state -> int32 array; None: trees 0 .. min(15, T) - 1, the reference's initial state (todos.txt:336-340)."""
        if state is None:
            state = range(min(15, self.forest_info()["n_trees"]))
        return np.ascontiguousarray(np.asarray(list(state), np.int32).reshape(-1))

    def forest_prune(self, X, labels=None, layer=0, state=None, params=None, **kw):
        """rvseg_forest_prune: simulated annealing over lists of the loaded forest's trees.  params: a
        capi.RvsegPruneParams, or its fields by keyword over the reference's defaults.  Returns dict(state int32 (the best
        state), best_energy float32, trace (structured: iteration, temperature, energy, best_energy, state_size -- one row
        per temperature iteration), step_kind uint8 (one per proposal: 0 rejected, 1 accepted, 2 accepted uphill))."""
        X = np.ascontiguousarray(X, np.float32)
        P, D = X.shape
        pp = params if params is not None else capi.prune_params(**kw)
        lab = None if labels is None else np.ascontiguousarray(np.asarray(labels, np.int32).reshape(-1))
        assert lab is None or lab.shape == (P,)
        first = self._prune_state(state)
        buf = np.zeros(capi.PRUNE_MAX_STATE, np.int32)
        n = C.c_int32(min(first.size, capi.PRUNE_MAX_STATE + 1))
        buf[:min(first.size, capi.PRUNE_MAX_STATE)] = first[:capi.PRUNE_MAX_STATE]
        try:
            iterations, steps = capi.prune_schedule(pp)
        except capi.RvsegError:
            iterations, steps = 0, 0          # the call below refuses it, with the library's message
        trace = np.zeros(iterations, np.dtype([("iteration", np.int32), ("temperature", np.float32), ("energy", np.float32),
                                               ("best_energy", np.float32), ("state_size", np.int32)]))
        kinds = np.zeros(steps, np.uint8)
        best, n_trace = C.c_float(), C.c_int32()
        capi.check(self.h, self.L.rvseg_forest_prune(self.h, _ptr(X), P, D, _ptr(lab), layer, C.byref(pp), _ptr(buf), C.byref(n), C.byref(best),
                                                     _ptr(trace), iterations, C.byref(n_trace), _ptr(kinds)))
        return {"state": buf[:n.value].copy(), "best_energy": np.float32(best.value), "trace": trace[:n_trace.value], "step_kind": kinds}

    def forest_prune_energy(self, X, labels, state, layer=0, energy=capi.PRUNE_ERROR):
        """rvseg_forest_prune_energy: the energy of one state (a list of tree indices) -> float32."""
        X = np.ascontiguousarray(X, np.float32)
        P, D = X.shape
        lab = None if labels is None else np.ascontiguousarray(np.asarray(labels, np.int32).reshape(-1))
        state = self._prune_state(state)
        out = C.c_float()
        capi.check(self.h, self.L.rvseg_forest_prune_energy(self.h, _ptr(X), P, D, _ptr(lab), layer, energy, _ptr(state), state.size, C.byref(out)))
        return np.float32(out.value)

    def forest_prune_apply(self, state):
        """rvseg_forest_prune_apply: the context's model becomes the forest of those trees, in that order."""
        state = self._prune_state(state)
        capi.check(self.h, self.L.rvseg_forest_prune_apply(self.h, _ptr(state), state.size))

    # ---- features ----------------------------------------------------------------------------
    def extract_features(self, rgb, depth, calib):
        p = self.params
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        calib = np.ascontiguousarray(calib, np.float32)
        assert rgb.shape == (p.height, p.width, 3) and depth.shape == (p.height, p.width) and calib.size == 21
        cap = (p.height // p.stride + 1) * (p.width // p.stride + 1)
        D = self.feature_length
        feat = np.empty((cap, D), np.float32)
        xv = np.empty(cap, np.int32)
        yv = np.empty(cap, np.int32)
        n = C.c_int32()
        capi.check(self.h, self.L.rvseg_extract_features(self.h, _ptr(rgb), _ptr(depth), _ptr(calib), _ptr(feat), _ptr(xv), _ptr(yv), C.byref(n)))
        return feat[:n.value].copy(), xv[:n.value].copy(), yv[:n.value].copy()

    # ---- whole path --------------------------------------------------------------------------
    def host_buffers(self, n, want_posteriors=True, want_marginals=None, want_labels=True):
        """Page-locked (rvseg_host_register) in / out buffers for calls of n frames: pass them to segment_frames(out=...)
        and reuse them across calls; free with release_host_buffers."""
        p = self.params
        cc = self.forest_info()["class_counts"]
        S, Lc, N = sum(cc), len(cc), p.width * p.height
        if want_marginals is None:
            want_marginals = bool(p.use_dense_crf)
        bufs = {"rgb": np.empty((n, p.height, p.width, 3), np.uint8), "depth": np.empty((n, p.height, p.width), np.uint16),
                "posteriors": np.empty((n, S * N), np.float32) if want_posteriors else None,
                "marginals": np.empty((n, S * N), np.float32) if want_marginals else None,
                "labels": np.empty((n, Lc, p.height, p.width), np.int8) if want_labels else None, "class_counts": cc}
        for k in ("rgb", "depth", "posteriors", "marginals", "labels"):
            if bufs[k] is not None:
                st = self.L.rvseg_host_register(_ptr(bufs[k]), bufs[k].nbytes)
                if st != capi.OK:
                    raise capi.RvsegError(st, "rvseg_host_register failed")
        return bufs

    def release_host_buffers(self, bufs):
        for k in ("rgb", "depth", "posteriors", "marginals", "labels"):
            if bufs.get(k) is not None:
                self.L.rvseg_host_unregister(_ptr(bufs[k]))

    def segment_frames(self, rgb, depth, calib, want_posteriors=True, want_marginals=None, want_labels=True, out=None):
        """out: buffers from host_buffers() (page-locked): results land there without a staging copy; rgb / depth may be
        out["rgb"] / out["depth"] themselves."""
        p = self.params
        if out is not None:
            n = rgb.shape[0]
            calib = np.ascontiguousarray(np.broadcast_to(np.asarray(calib, np.float32).reshape(-1, 21), (n, 21)))
            capi.check(self.h, self.L.rvseg_segment_frames(self.h, n, _ptr(rgb), _ptr(depth), _ptr(calib), _ptr(out["posteriors"]),
                                                           _ptr(out["marginals"]), _ptr(out["labels"])))
            return out
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        n = rgb.shape[0]
        assert rgb.shape == (n, p.height, p.width, 3) and depth.shape == (n, p.height, p.width)
        calib = np.ascontiguousarray(np.broadcast_to(np.asarray(calib, np.float32).reshape(-1, 21), (n, 21)))
        cc = self.forest_info()["class_counts"]
        S, Lc, N = sum(cc), len(cc), p.width * p.height
        if want_marginals is None:
            want_marginals = bool(p.use_dense_crf)
        post = np.empty((n, S * N), np.float32) if want_posteriors else None
        marg = np.empty((n, S * N), np.float32) if want_marginals else None
        lab = np.empty((n, Lc, p.height, p.width), np.int8) if want_labels else None
        capi.check(self.h, self.L.rvseg_segment_frames(self.h, n, _ptr(rgb), _ptr(depth), _ptr(calib), _ptr(post), _ptr(marg), _ptr(lab)))
        return {"posteriors": post, "marginals": marg, "labels": lab, "class_counts": cc}

    def segment_frames_device(self, n, d_rgb, d_depth, calib, d_post=0, d_marg=0, d_labels=0, stream=0):
        """Device-pointer variant: integer addresses (e.g. torch tensor.data_ptr()) and a raw
        hipStream_t handle.  Enqueues only; the caller synchronises."""
        calib = np.ascontiguousarray(np.broadcast_to(np.asarray(calib, np.float32).reshape(-1, 21), (n, 21)))
        capi.check(self.h, self.L.rvseg_segment_frames_device(
            self.h, n, C.c_void_p(d_rgb), C.c_void_p(d_depth), _ptr(calib),
            C.c_void_p(d_post or None), C.c_void_p(d_marg or None), C.c_void_p(d_labels or None),
            C.c_void_p(stream or None)))

    # ---- external semantics (src/segmenter.cpp:445-514) --------------------------------------------
    def rectify_depth(self, depth, calib, depth_min=0.5, depth_max=15.0):
        """rvseg_rectify_depth: depth (n, H, W) uint16 mm -> (n, H, W, 3) float32, the TYPE_32FC3 `depth` image of a
        SingleFrameSegmentation request; NaN outside [depth_min, depth_max] (the reference's 0.5 / 15.0 by default)."""
        p = self.params
        depth = np.ascontiguousarray(depth, np.uint16)
        n = depth.shape[0]
        assert depth.shape == (n, p.height, p.width)
        calib = np.ascontiguousarray(np.broadcast_to(np.asarray(calib, np.float32).reshape(-1, 21), (n, 21)))
        out = np.empty((n, p.height, p.width, 3), np.float32)
        capi.check(self.h, self.L.rvseg_rectify_depth(self.h, n, _ptr(depth), _ptr(calib), C.c_float(depth_min), C.c_float(depth_max), _ptr(out)))
        return out

    def rectify_depth_device(self, n, d_depth, calib, d_xyz, depth_min=0.5, depth_max=15.0, stream=0):
        """Device-pointer variant (integer addresses): enqueues only."""
        calib = np.ascontiguousarray(np.broadcast_to(np.asarray(calib, np.float32).reshape(-1, 21), (n, 21)))
        capi.check(self.h, self.L.rvseg_rectify_depth_device(self.h, n, C.c_void_p(d_depth), _ptr(calib), C.c_float(depth_min),
                                                             C.c_float(depth_max), C.c_void_p(d_xyz), C.c_void_p(stream or None)))

    def external_layers_set(self, class_counts):
        """rvseg_external_layers_set: the layer layout of the external provider's distributions."""
        cc = [int(c) for c in class_counts]
        arr = (C.c_int32 * max(1, len(cc)))(*cc)
        capi.check(self.h, self.L.rvseg_external_layers_set(self.h, len(cc), arr))
        self.external_class_counts = cc

    def segment_external(self, rgb, depth, calib, distributions, dist_stride=1, want_marginals=None, want_labels=True):
        """rvseg_segment_external: distributions (n, S * h * w) float32 with h x w = H x W (dist_stride 1) or
        H/stride x W/stride (dist_stride == params.stride), per frame [layer][y][x][class].  Returns marginals (with
        use_dense_crf) and labels like segment_frames."""
        p = self.params
        cc = getattr(self, "external_class_counts", None)
        if cc is None:
            capi.check(self.h, self.L.rvseg_segment_external(self.h, 0, None, None, None, None, dist_stride, None, None))   # raises: no layout
            raise capi.RvsegError(capi.ERR_INVALID_ARG, "no external layer layout set")
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        n = rgb.shape[0]
        assert rgb.shape == (n, p.height, p.width, 3) and depth.shape == (n, p.height, p.width)
        calib = np.ascontiguousarray(np.broadcast_to(np.asarray(calib, np.float32).reshape(-1, 21), (n, 21)))
        S, Lc, N = sum(cc), len(cc), p.width * p.height
        dist = np.ascontiguousarray(distributions, np.float32).reshape(n, -1)
        if dist_stride in (1, p.stride):   # any other stride is the library's to refuse
            assert dist.shape[1] == S * (N if dist_stride == 1 else (p.height // p.stride) * (p.width // p.stride)), dist.shape
        if want_marginals is None:
            want_marginals = bool(p.use_dense_crf)
        marg = np.empty((n, S * N), np.float32) if want_marginals else None
        lab = np.empty((n, Lc, p.height, p.width), np.int8) if want_labels else None
        capi.check(self.h, self.L.rvseg_segment_external(self.h, n, _ptr(rgb), _ptr(depth), _ptr(calib), _ptr(dist), dist_stride,
                                                         _ptr(marg), _ptr(lab)))
        return {"marginals": marg, "labels": lab, "class_counts": list(cc)}

    def segment_external_device(self, n, d_rgb, d_depth, calib, d_dist, dist_stride=1, d_marg=0, d_labels=0, stream=0):
        """Device-pointer variant (integer addresses): enqueues only; the caller synchronises and polls (poll_status)."""
        calib = np.ascontiguousarray(np.broadcast_to(np.asarray(calib, np.float32).reshape(-1, 21), (n, 21)))
        capi.check(self.h, self.L.rvseg_segment_external_device(
            self.h, n, C.c_void_p(d_rgb or None), C.c_void_p(d_depth or None), _ptr(calib), C.c_void_p(d_dist or None), dist_stride,
            C.c_void_p(d_marg or None), C.c_void_p(d_labels or None), C.c_void_p(stream or None)))

    # ---- CRF ---------------------------------------------------------------------------------
    def crf_infer(self, unary_energy, features, potts_w, iterations, label_mode=capi.LABEL_ARGMAX, unknown_label=0):
        U = np.ascontiguousarray(unary_energy, np.float32)
        F = np.ascontiguousarray(features, np.float32)
        N, Cn = U.shape
        assert F.shape[0] == N
        Q = np.empty_like(U)
        mp = np.empty(N, np.int8)
        capi.check(self.h, self.L.rvseg_crf_infer(self.h, N, Cn, F.shape[1], _ptr(U), _ptr(F), C.c_float(potts_w), iterations, _ptr(Q), _ptr(mp), label_mode, unknown_label))
        return Q, mp

    def crf_infer_multi(self, unary_energy, features, ws, iterations, label_mode=capi.LABEL_ARGMAX, unknown_label=0):
        U = np.ascontiguousarray(unary_energy, np.float32)
        N, Cn = U.shape
        feats = [np.ascontiguousarray(f, np.float32) for f in features]
        ds = (C.c_int32 * len(feats))(*[f.shape[1] for f in feats])
        ptrs = (C.c_void_p * len(feats))(*[f.ctypes.data for f in feats])
        wsa = (C.c_float * len(feats))(*ws)
        Q = np.empty_like(U)
        mp = np.empty(N, np.int8)
        capi.check(self.h, self.L.rvseg_crf_infer_multi(self.h, N, Cn, len(feats), ds, ptrs, wsa, _ptr(U), iterations, _ptr(Q), _ptr(mp), label_mode, unknown_label))
        return Q, mp

    def crf_infer_terms(self, unary_energy, terms, iterations, label_mode=capi.LABEL_ARGMAX, unknown_label=0):
        """rvseg_crf_infer_terms.  terms: [(features N x d, compatibility, kernel_type, normalization, kernel_params or None)];
        a compatibility is a float (Potts weight) or a Potts / Diagonal / MatrixCompatibility."""
        U = np.ascontiguousarray(unary_energy, np.float32)
        N, Cn = U.shape
        arr, keep = _crf_terms(terms, Cn, N)
        Q = np.empty_like(U)
        mp = np.empty(N, np.int8)
        capi.check(self.h, self.L.rvseg_crf_infer_terms(self.h, N, Cn, len(terms), arr, _ptr(U), iterations, _ptr(Q), _ptr(mp),
                                                        label_mode, unknown_label))
        del keep
        return Q, mp

    def crf_infer_terms_device(self, N, Cn, terms, d_unary, unary_is_energy, iterations, d_Q=0, d_map=0,
                               label_mode=capi.LABEL_ARGMAX, unknown_label=0, stream=0):
        """rvseg_crf_infer_terms_device: the term features are integer device addresses (N x d each), enqueues only."""
        arr, keep = _crf_terms(terms, Cn, N, device=True)
        capi.check(self.h, self.L.rvseg_crf_infer_terms_device(
            self.h, N, Cn, len(terms), arr, C.c_void_p(d_unary), 1 if unary_is_energy else 0, iterations,
            C.c_void_p(d_Q or None), C.c_void_p(d_map or None), label_mode, unknown_label, C.c_void_p(stream or None)))
        del keep

    def crf_logistic_unary(self, L, f):
        """LogisticUnaryEnergy::get (unary.cpp:50-52): L (C x K), f (N x K) -> the energy U (N x C)."""
        Lm = np.ascontiguousarray(L, np.float32)
        F = np.ascontiguousarray(f, np.float32)
        Cn, K = Lm.shape
        N = F.shape[0]
        assert F.shape == (N, K)
        U = np.empty((N, Cn), np.float32)
        capi.check(self.h, self.L.rvseg_crf_logistic_unary(self.h, N, Cn, K, _ptr(Lm), _ptr(F), _ptr(U)))
        return U

    def crf_logistic_unary_device(self, N, L, d_f, d_U, stream=0):
        Lm = np.ascontiguousarray(L, np.float32)
        Cn, K = Lm.shape
        capi.check(self.h, self.L.rvseg_crf_logistic_unary_device(self.h, N, Cn, K, _ptr(Lm), C.c_void_p(d_f), C.c_void_p(d_U),
                                                                  C.c_void_p(stream or None)))

    # ---- a DenseCRF kept on the context (rvseg_crf_model_*): the state of this context until its next lattice build.  Which
    # model it is and its shape are the library's to say (rvseg_crf_model_info): nothing of it is recorded here ----
    def crf_model_set(self, unary, terms, unary_is_energy=True):
        """rvseg_crf_model_set: terms as for crf_infer_terms; the arrays are free once this returns.  Returns the serial of
        the new model (crf_model_serial)."""
        U = np.ascontiguousarray(unary, np.float32)
        N, Cn = U.shape
        arr, keep = _crf_terms(terms, Cn, N)
        capi.check(self.h, self.L.rvseg_crf_model_set(self.h, N, Cn, len(terms), arr, _ptr(U), 1 if unary_is_energy else 0))
        del keep
        return self.crf_model_serial()

    def crf_model_set_device(self, N, Cn, terms, d_unary, unary_is_energy=True, stream=0):
        arr, keep = _crf_terms(terms, Cn, N, device=True)
        capi.check(self.h, self.L.rvseg_crf_model_set_device(self.h, N, Cn, len(terms), arr, C.c_void_p(d_unary), 1 if unary_is_energy else 0,
                                                             C.c_void_p(stream or None)))
        del keep
        return self.crf_model_serial()

    def _crf_model(self):
        """struct rvseg_crf_model_info of the live model; without one, the library's refusal (it names what replaced it)."""
        info = capi.RvsegCrfModelInfo()
        capi.check(self.h, self.L.rvseg_crf_model_info(self.h, C.byref(info)))
        return info

    def crf_model_serial(self):
        """The serial of the live model: every crf_model_set[_device] of the process gives a new one, the in-place setters
        keep it.  0 without a live model."""
        info = capi.RvsegCrfModelInfo()
        self.L.rvseg_crf_model_info(self.h, C.byref(info))   # (zeroes info when it refuses)
        return int(info.serial)

    @staticmethod
    def _model_matrix(m, Q, copy=False):
        """Q as a C-contiguous float32 N x C matrix of the model m; copy: never the caller's array."""
        Q = np.array(Q, np.float32, order="C") if copy else np.ascontiguousarray(Q, np.float32)
        assert Q.shape == (m.N, m.C)
        return Q

    def crf_model_start(self):
        m = self._crf_model()
        Q = np.empty((m.N, m.C), np.float32)
        capi.check(self.h, self.L.rvseg_crf_model_start(self.h, _ptr(Q)))
        return Q

    def crf_model_step(self, Q, n_steps=1):
        """n_steps of stepInference on a copy of Q (any N x C matrix), which is returned."""
        Q = self._model_matrix(self._crf_model(), Q, copy=True)
        capi.check(self.h, self.L.rvseg_crf_model_step(self.h, _ptr(Q), n_steps))
        return Q

    def _model_map(self, fn, term, Q):
        """One of the entries that take a term and an N x C matrix and give an N x C matrix."""
        Q = self._model_matrix(self._crf_model(), Q)
        out = np.empty_like(Q)
        capi.check(self.h, fn(self.h, term, _ptr(Q), _ptr(out)))
        return out

    def crf_model_apply(self, term, Q):
        return self._model_map(self.L.rvseg_crf_model_apply, term, Q)

    def crf_model_energy(self, labels, term=-1, unary=True, pairwise=True):
        """(unary energy, pairwise energy) per point of a labelling (int8, N); a part not asked for is None."""
        N = self._crf_model().N
        lab = np.ascontiguousarray(labels, np.int8)
        assert lab.shape == (N,)
        u = np.empty(N, np.float32) if unary else None
        p = np.empty(N, np.float32) if pairwise else None
        capi.check(self.h, self.L.rvseg_crf_model_energy(self.h, _ptr(lab), term, _ptr(u), _ptr(p)))
        return u, p

    def crf_model_kl(self, Q):
        """The parts of the KL divergence: entropy, unary, one per term (float64); their sum in that order is the KL."""
        m = self._crf_model()
        Q = self._model_matrix(m, Q)
        parts = np.empty(2 + m.n_terms, np.float64)
        capi.check(self.h, self.L.rvseg_crf_model_kl(self.h, _ptr(Q), _ptr(parts)))
        return parts

    def crf_model_trace(self, iterations, label_mode=capi.LABEL_ARGMAX, unknown_label=0):
        """Inference from the start: (Q, map, kl) with kl[it] the KL divergence after the start and after every iteration."""
        m = self._crf_model()
        Q = np.empty((m.N, m.C), np.float32)
        mp = np.empty(m.N, np.int8)
        kl = np.empty(iterations + 1, np.float64)
        capi.check(self.h, self.L.rvseg_crf_model_trace(self.h, iterations, _ptr(Q), _ptr(mp), label_mode, unknown_label, _ptr(kl)))
        return Q, mp, kl

    # ---- learning on the kept model (rvseg.h, "Learning on the kept model") ----
    def crf_model_apply_transpose(self, term, Q):
        return self._model_map(self.L.rvseg_crf_model_apply_transpose, term, Q)

    def crf_model_objective(self, objective, Q):
        """(value, d_mul_Q) of a LogLikelihood / Hamming / IntersectionOverUnion on the marginals Q."""
        Q = self._model_matrix(self._crf_model(), Q)
        rec, keep = objective.record(*Q.shape)
        value = np.empty(1, np.float64)
        dq = np.empty_like(Q)
        capi.check(self.h, self.L.rvseg_crf_model_objective(self.h, C.byref(rec), _ptr(Q), _ptr(value), _ptr(dq)))
        del keep
        return float(value[0]), dq

    def _model_grads(self, m, unary, lbl_cmp, kernel, call):
        """The optional gradient outputs of a backward / gradient entry on the model m: allocated as asked for, handed to
        call(unary_grad, compat_grad, kernel_grad) as pointers (NULL: not asked for) and returned trimmed to the model's
        counts, None where not asked for.  unary: False, True (N x C float32) or "params" (the C K doubles of a kept
        logistic unary).  The doubles are never an empty array, whose pointer would say "not asked for"."""
        sizes = (m.C * m.K, m.n_compat_params, m.n_kernel_params)
        outs = [np.zeros(max(1, n), np.float64) if want else None for n, want in zip(sizes, (unary == "params", lbl_cmp, kernel))]
        if unary and unary != "params":
            outs[0] = np.empty((m.N, m.C), np.float32)
        capi.check(self.h, call(*[_ptr(o) for o in outs]))
        return tuple(o if o is None or o.ndim == 2 else o[:n] for o, n in zip(outs, sizes))

    def _model_backward(self, fn, Q_all, d_mul_Q, unary, lbl_cmp, kernel):
        """(unary_grad, compat_grad, kernel_grad) of a backward entry; kernel None: fn takes no kernel gradient."""
        m = self._crf_model()
        Q_all = np.ascontiguousarray(Q_all, np.float32)
        dq = self._model_matrix(m, d_mul_Q)
        assert Q_all.ndim == 3 and Q_all.shape[1:] == (m.N, m.C)
        return self._model_grads(m, unary, lbl_cmp, kernel, lambda ug, cg, kg: fn(
            self.h, Q_all.shape[0] - 1, _ptr(Q_all), _ptr(dq), ug, cg, *(() if kernel is None else (kg,))))

    def _model_gradient(self, fn, iterations, objective, unary, lbl_cmp, kernel, want_Q):
        """(value, unary_grad, compat_grad, kernel_grad, Q[n]) of a gradient entry; kernel / want_Q None: fn has no such
        argument."""
        m = self._crf_model()
        rec, keep = objective.record(m.N, m.C)
        value = np.empty(1, np.float64)
        Q = np.empty((m.N, m.C), np.float32) if want_Q else None
        grads = self._model_grads(m, unary, lbl_cmp, kernel, lambda ug, cg, kg: fn(
            self.h, iterations, C.byref(rec), _ptr(value), ug, cg, *(() if kernel is None else (kg,)), *(() if want_Q is None else (_ptr(Q),))))
        del keep
        return (float(value[0]),) + grads + (Q,)

    def crf_model_backward(self, Q_all, d_mul_Q, unary=True, lbl_cmp=True):
        """(unary_grad N x C float32, compat_grad float64) from Q[0 .. n] ((n + 1) x N x C) and d_mul_Q; a part not asked
        for is None."""
        return self._model_backward(self.L.rvseg_crf_model_backward, Q_all, d_mul_Q, bool(unary), lbl_cmp, None)[:2]

    def crf_model_gradient(self, iterations, objective, unary=True, lbl_cmp=True, want_Q=False):
        """rvseg_crf_model_gradient: (value, unary_grad, compat_grad, Q[n]); a part not asked for is None."""
        value, ug, cg, _, Q = self._model_gradient(self.L.rvseg_crf_model_gradient, iterations, objective, bool(unary), lbl_cmp, None,
                                                   bool(want_Q))
        return value, ug, cg, Q

    # ---- the kernel-parameter gradient (rvseg.h, "Kernel-parameter gradient") ----
    def crf_model_compat_apply(self, term, Q):
        """lbl_Q: the term's compatibility on Q (N x C) with no filter (pairwise.cpp:203-205)."""
        return self._model_map(self.L.rvseg_crf_model_compat_apply, term, Q)

    def crf_model_lattice_gradient(self, term, a, b):
        """Permutohedral::gradient(a, b) of a term's lattice with respect to its features, N x d float32 (a, b: N x C)."""
        m = self._crf_model()
        a, b = self._model_matrix(m, a), self._model_matrix(m, b)
        df = np.empty((m.N, m.d[term] if 0 <= term < m.n_terms else 1), np.float32)   # (no such term: the library refuses)
        capi.check(self.h, self.L.rvseg_crf_model_lattice_gradient(self.h, term, _ptr(a), _ptr(b), _ptr(df)))
        return df

    def crf_model_kernel_gradient(self, term, a, b, want_fg=False):
        """DenseKernel::gradient(a, b) of a term: float64 (CONST 0, DIAG d, FULL d x d column-major values); want_fg: (that,
        featureGradient N x d float32)."""
        m = self._crf_model()
        a, b = self._model_matrix(m, a), self._model_matrix(m, b)
        ok = 0 <= term < m.n_terms   # (no such term: the library refuses)
        n = m.kernel_params[term] if ok else 0
        grad = np.zeros(max(1, n), np.float64)
        fg = np.empty((m.N, m.d[term] if ok else 1), np.float32) if want_fg else None
        capi.check(self.h, self.L.rvseg_crf_model_kernel_gradient(self.h, term, _ptr(a), _ptr(b), _ptr(grad), _ptr(fg)))
        return (grad[:n], fg) if want_fg else grad[:n]

    def crf_model_backward_kernel(self, Q_all, d_mul_Q, unary=True, lbl_cmp=True, kernel=True):
        """crf_model_backward with the kernel-parameter gradient (float64, the layout of kernelParameters()) as a third
        element; a part not asked for is None."""
        return self._model_backward(self.L.rvseg_crf_model_backward_kernel, Q_all, d_mul_Q, bool(unary), lbl_cmp, bool(kernel))

    def crf_model_gradient_kernel(self, iterations, objective, unary=True, lbl_cmp=True, kernel=True, want_Q=False):
        """rvseg_crf_model_gradient_kernel: (value, unary_grad, compat_grad, kernel_grad, Q[n]); a part not asked for is None."""
        return self._model_gradient(self.L.rvseg_crf_model_gradient_kernel, iterations, objective, bool(unary), lbl_cmp, bool(kernel),
                                    bool(want_Q))

    def crf_model_set_compat(self, term, compatibility):
        """Replaces the parameters of a term's compatibility (same kind) in the live model: no lattice build."""
        cp = np.ascontiguousarray(_compat(compatibility).array(self._crf_model().C), np.float32)
        capi.check(self.h, self.L.rvseg_crf_model_set_compat(self.h, term, _ptr(cp)))

    def crf_model_set_unary(self, unary, unary_is_energy=True):
        U = self._model_matrix(self._crf_model(), unary)
        capi.check(self.h, self.L.rvseg_crf_model_set_unary(self.h, _ptr(U), 1 if unary_is_energy else 0))

    # ---- the learning loop (rvseg.h, "The learning loop") ----
    def crf_model_set_kernel(self, term, params):
        """Rebuilds one DIAG / FULL term's lattice in the live model from the features it keeps; params None: the features
        as passed."""
        m = self._crf_model()
        kp = None if params is None else np.ascontiguousarray(params, np.float32).reshape(-1)
        if kp is not None and 0 <= term < m.n_terms:   # (no such term: the library refuses)
            assert kp.shape == (m.kernel_params[term],)
        capi.check(self.h, self.L.rvseg_crf_model_set_kernel(self.h, term, _ptr(kp)))

    def crf_model_set_logistic(self, L, f):
        """The live model keeps f (N x K) and its unary becomes the energy L f (L: C x K)."""
        m = self._crf_model()
        Lm = np.ascontiguousarray(L, np.float32)
        F = np.ascontiguousarray(f, np.float32)
        assert Lm.ndim == 2 and Lm.shape[0] == m.C and F.shape == (m.N, Lm.shape[1])
        capi.check(self.h, self.L.rvseg_crf_model_set_logistic(self.h, Lm.shape[1], _ptr(Lm), _ptr(F)))

    def crf_model_set_logistic_device(self, L, d_f, stream=0):
        Lm = np.ascontiguousarray(L, np.float32)
        assert Lm.ndim == 2 and Lm.shape[0] == self._crf_model().C
        self.crf_model_call_device("set_logistic", Lm.shape[1], Lm.ctypes.data, d_f, stream=stream)

    def crf_model_set_logistic_params(self, L):
        m = self._crf_model()
        Lm = np.ascontiguousarray(L, np.float32)
        assert Lm.ndim == 2 and Lm.shape[0] == m.C and (m.K == 0 or Lm.shape[1] == m.K)   # (K == 0: the library refuses)
        capi.check(self.h, self.L.rvseg_crf_model_set_logistic_params(self.h, _ptr(Lm)))

    def crf_model_gradient_params(self, iterations, objective, unary=True, lbl_cmp=True, kernel=True):
        """rvseg_crf_model_gradient_params: (value, unary_grad C K float64 column-major, compat_grad, kernel_grad); a part not
        asked for is None."""
        return self._model_gradient(self.L.rvseg_crf_model_gradient_params, iterations, objective, "params" if unary else False, lbl_cmp,
                                    bool(kernel), None)[:4]

    def crf_model_energy_gradient(self, iterations, objective, learn_mask, l2_norm, x):
        """rvseg_crf_model_energy_gradient: CRFEnergy::gradient on the live model -> (value, dx float32)."""
        m = self._crf_model()
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        rec, keep = objective.record(m.N, m.C)
        value = np.empty(1, np.float64)
        dx = np.zeros(max(1, x.shape[0]), np.float32)
        capi.check(self.h, self.L.rvseg_crf_model_energy_gradient(self.h, iterations, C.byref(rec), int(learn_mask), C.c_float(float(l2_norm)),
                                                                  _ptr(x if x.shape[0] else dx), x.shape[0], _ptr(value), _ptr(dx)))
        del keep
        return float(value[0]), dx[:x.shape[0]]

    def crf_logistic_gradient(self, unary_grad, f):
        """LogisticUnaryEnergy::gradient (unary.cpp:64-68): unary_grad (N x C), f (N x K) -> C K doubles, column-major like
        unaryParameters()."""
        g = np.ascontiguousarray(unary_grad, np.float32)
        F = np.ascontiguousarray(f, np.float32)
        N, Cn = g.shape
        K = F.shape[1]
        assert F.shape == (N, K)
        out = np.empty(Cn * K, np.float64)
        capi.check(self.h, self.L.rvseg_crf_logistic_gradient(self.h, N, Cn, K, _ptr(g), _ptr(F), _ptr(out)))
        return out

    def crf_logistic_gradient_device(self, N, Cn, K, d_unary_grad, d_f, d_out, stream=0):
        capi.check(self.h, self.L.rvseg_crf_logistic_gradient_device(self.h, N, Cn, K, C.c_void_p(d_unary_grad), C.c_void_p(d_f),
                                                                     C.c_void_p(d_out), C.c_void_p(stream or None)))

    def crf_model_call_device(self, name, *args, stream=0):
        """rvseg_crf_model_<name>_device with integer device addresses / integers as in rvseg.h, the stream last; enqueues only."""
        fn = getattr(self.L, "rvseg_crf_model_%s_device" % name)
        conv = [C.c_void_p(a or None) if t is C.c_void_p else a for a, t in zip(args, fn.argtypes[1:])]
        capi.check(self.h, fn(self.h, *conv, C.c_void_p(stream or None)))

    # ---- local-map fusion -------------------------------------------------------------------
    def fuse_posteriors(self, index_images, posteriors, class_counts, cloud_size):
        p = self.params
        idx = np.ascontiguousarray(index_images, np.int32)
        n = idx.shape[0]
        assert idx.shape == (n, p.height, p.width)
        S = int(sum(class_counts))
        post = np.ascontiguousarray(posteriors, np.float32).reshape(n, S * p.height * p.width)
        cc = (C.c_int32 * len(class_counts))(*class_counts)
        out = np.empty(cloud_size * S, np.float32)
        capi.check(self.h, self.L.rvseg_fuse_posteriors(self.h, n, _ptr(idx), _ptr(post), len(class_counts), cc, cloud_size, _ptr(out)))
        return out

    def process_map_device(self, n_images, d_index_images, d_posteriors, cloud_size, d_cloud_xyz, d_cloud_rgb, d_labels,
                           d_unaries=0, stream=0):
        """rvseg_process_map_device: integer device addresses, enqueues only."""
        capi.check(self.h, self.L.rvseg_process_map_device(
            self.h, n_images, C.c_void_p(d_index_images), C.c_void_p(d_posteriors), cloud_size,
            C.c_void_p(d_cloud_xyz or None), C.c_void_p(d_cloud_rgb or None), C.c_void_p(d_labels),
            C.c_void_p(d_unaries or None), C.c_void_p(stream or None)))

    # ---- projector: index images from poses (src/segmenter.cpp:234-240, 576-578) --------------------------
    @staticmethod
    def _projections(projections):
        P = np.ascontiguousarray(projections, np.float32)
        if P.size % 12:
            raise ValueError("projections: n_images x 3 x 4 floats")
        return P.reshape(-1, 12)

    def project_cloud(self, projections, cloud_xyz, want_zbuffer=True):
        """rvseg_project_cloud: projections (n, 3, 4) float32 (map frame -> homogeneous pixels), cloud_xyz (N, 3).
        Returns (index (n, H, W) int32 with -1 = no point, zbuffer (n, H, W) float32 with +inf = no point, or None)."""
        p = self.params
        P = self._projections(projections)
        xyz = np.ascontiguousarray(cloud_xyz, np.float32).reshape(-1, 3)
        n = P.shape[0]
        idx = np.full((n, p.height, p.width), -1, np.int32)
        z = np.full((n, p.height, p.width), np.inf, np.float32) if want_zbuffer else None
        capi.check(self.h, self.L.rvseg_project_cloud(self.h, n, _ptr(P), xyz.shape[0], _ptr(xyz), _ptr(idx), _ptr(z)))
        return idx, z

    def project_cloud_device(self, projections, N, d_cloud_xyz, d_index, d_zbuffer=0, stream=0):
        """rvseg_project_cloud_device: integer device addresses (the matrices stay a host array), enqueues only."""
        P = self._projections(projections)
        capi.check(self.h, self.L.rvseg_project_cloud_device(self.h, P.shape[0], _ptr(P), N, C.c_void_p(d_cloud_xyz or None),
                                                             C.c_void_p(d_index or None), C.c_void_p(d_zbuffer or None),
                                                             C.c_void_p(stream or None)))

    def process_map_poses_device(self, projections, d_posteriors, cloud_size, d_cloud_xyz, d_cloud_rgb, d_labels, d_unaries=0,
                                 d_index=0, stream=0):
        """rvseg_process_map_poses_device: process_map_device with the index images made by the projector."""
        P = self._projections(projections)
        capi.check(self.h, self.L.rvseg_process_map_poses_device(
            self.h, P.shape[0], _ptr(P), C.c_void_p(d_posteriors or None), cloud_size, C.c_void_p(d_cloud_xyz or None),
            C.c_void_p(d_cloud_rgb or None), C.c_void_p(d_labels or None), C.c_void_p(d_unaries or None), C.c_void_p(d_index or None),
            C.c_void_p(stream or None)))

    def crf_infer_device(self, N, Cn, d, d_unary, unary_is_energy, d_features, potts_w, iterations, d_Q=0, d_map=0,
                         label_mode=capi.LABEL_ARGMAX, unknown_label=0, stream=0):
        capi.check(self.h, self.L.rvseg_crf_infer_device(
            self.h, N, Cn, d, C.c_void_p(d_unary), 1 if unary_is_energy else 0, C.c_void_p(d_features), C.c_float(potts_w),
            iterations, C.c_void_p(d_Q or None), C.c_void_p(d_map or None), label_mode, unknown_label, C.c_void_p(stream or None)))

    # ---- multi-GPU local-map gather over RCCL ------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        st = capi.lib().rvseg_comm_unique_id(buf)
        if st != capi.OK:
            raise capi.RvsegError(st, "rvseg_comm_unique_id failed (librccl.so missing?)")
        return buf.raw

    def comm_init(self, rank, world, unique_id):
        capi.check(self.h, self.L.rvseg_comm_init(self.h, rank, world, bytes(unique_id)))

    def gather_frames(self, d_local, bytes_per_rank, d_recv=0, root=0, stream=0):
        capi.check(self.h, self.L.rvseg_gather_frames(self.h, C.c_void_p(d_local), bytes_per_rank, C.c_void_p(d_recv or None), root,
                                                      C.c_void_p(stream or None)))

    def label_values(self, values, label_mode, unknown_label=0):
        V = np.ascontiguousarray(values, np.float32)
        N, Cn = V.shape
        out = np.empty(N, np.int8)
        capi.check(self.h, self.L.rvseg_label_values(self.h, _ptr(V), N, Cn, label_mode, unknown_label, _ptr(out)))
        return out

    def lattice_build(self, features, keys_capacity=None):
        F = np.ascontiguousarray(features, np.float32)
        N, d = F.shape
        cap = keys_capacity or N * (d + 1) + 8 * (d + 1)
        off = np.empty((N, d + 1), np.int32)
        bary = np.empty((N, d + 1), np.float32)
        keys = np.empty((cap, d), np.int16)
        M = C.c_int32()
        capi.check(self.h, self.L.rvseg_lattice_build(self.h, _ptr(F), N, d, _ptr(off), _ptr(bary), _ptr(keys), cap, C.byref(M)))
        return off, bary, keys[:M.value].copy(), M.value

    def lattice_neighbours(self, M, d, N):
        n1 = np.empty((d + 1, M), np.int32)
        n2 = np.empty((d + 1, M), np.int32)
        pix = np.empty(N * (d + 1), np.uint32)
        vs = np.empty(M, np.uint32)
        ve = np.empty(M, np.uint32)
        capi.check(self.h, self.L.rvseg_lattice_neighbours(self.h, _ptr(n1), _ptr(n2), _ptr(pix), _ptr(vs), _ptr(ve)))
        return n1, n2, pix, vs, ve

    def lattice_filter(self, values):
        V = np.ascontiguousarray(values, np.float32)
        out = np.empty_like(V)
        capi.check(self.h, self.L.rvseg_lattice_filter(self.h, _ptr(V), V.shape[1], _ptr(out)))
        return out

    # ---- scoring (colour-coded labels, confusion matrix; include/rvseg.h "scoring") -------------------------------
    def color_coding_set(self, layer, coding, missing_label=0):
        """rvseg_color_coding_set: `coding` is one config.json color_codings[*].coding list of {name, color, label}."""
        n = len(coding)
        rgb = np.array([[int(c) & 255 for c in e["color"]] for e in coding], np.uint8).reshape(n, 3)
        lab = np.array([int(e["label"]) for e in coding], np.int64).astype(np.int8)   # label_type = char (defines.h)
        capi.check(self.h, self.L.rvseg_color_coding_set(self.h, layer, n, _ptr(rgb), _ptr(lab), missing_label))

    def _label_image_shape(self, layer):
        p = self.params
        return (p.height, p.width) if layer >= 0 else (len(self.forest_info()["class_counts"]), p.height, p.width)

    def labels_from_rgb(self, rgb, layer=-1):
        """rvseg_labels_from_rgb: rgb (n, [L,] H, W, 3) uint8 -> (n, [L,] H, W) int8; layer < 0: every layer."""
        shp = self._label_image_shape(layer)
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.shape[1:] == shp + (3,), rgb.shape
        out = np.empty(rgb.shape[:-1], np.int8)
        capi.check(self.h, self.L.rvseg_labels_from_rgb(self.h, layer, rgb.shape[0], _ptr(rgb), _ptr(out)))
        return out

    def labels_to_rgb(self, labels, layer=-1):
        """rvseg_labels_to_rgb: (n, [L,] H, W) int8 -> (n, [L,] H, W, 3) uint8 (R, G, B bytes)."""
        shp = self._label_image_shape(layer)
        labels = np.ascontiguousarray(labels, np.int8)
        assert labels.shape[1:] == shp, labels.shape
        out = np.empty(labels.shape + (3,), np.uint8)
        capi.check(self.h, self.L.rvseg_labels_to_rgb(self.h, layer, labels.shape[0], _ptr(labels), _ptr(out)))
        return out

    def labels_from_rgb_device(self, n, d_rgb, d_labels, layer=-1, stream=0):
        capi.check(self.h, self.L.rvseg_labels_from_rgb_device(self.h, layer, n, C.c_void_p(d_rgb), C.c_void_p(d_labels),
                                                               C.c_void_p(stream or None)))

    def labels_to_rgb_device(self, n, d_labels, d_rgb, layer=-1, stream=0):
        capi.check(self.h, self.L.rvseg_labels_to_rgb_device(self.h, layer, n, C.c_void_p(d_labels), C.c_void_p(d_rgb),
                                                             C.c_void_p(stream or None)))

    def eval_reset(self):
        capi.check(self.h, self.L.rvseg_eval_reset(self.h))

    def eval_accumulate(self, pred, gt, gt_format=None):
        """rvseg_eval_accumulate: pred (n, L, H, W) int8; gt (n, L, H, W) int8 or (n, L, H, W, 3) uint8 colour codes.
        gt_format defaults by shape (capi.GT_RGB for the trailing 3)."""
        pred = np.ascontiguousarray(pred, np.int8)
        n = pred.shape[0]
        if gt_format is None:
            gt_format = capi.GT_RGB if np.ndim(gt) == pred.ndim + 1 else capi.GT_LABELS
        gt = np.ascontiguousarray(gt, np.uint8 if gt_format == capi.GT_RGB else np.int8)
        assert pred.shape == (n,) + self._label_image_shape(-1), pred.shape
        assert gt.shape == pred.shape + ((3,) if gt_format == capi.GT_RGB else ()), gt.shape
        capi.check(self.h, self.L.rvseg_eval_accumulate(self.h, n, _ptr(pred), _ptr(gt), gt_format))

    def eval_accumulate_device(self, n, d_pred, d_gt, gt_format=capi.GT_LABELS, stream=0):
        """rvseg_eval_accumulate_device: integer device addresses, enqueues only."""
        capi.check(self.h, self.L.rvseg_eval_accumulate_device(self.h, n, C.c_void_p(d_pred), C.c_void_p(d_gt), gt_format,
                                                               C.c_void_p(stream or None)))

    def eval_confusion(self, layer):
        """(C x C uint64 counts, out-of-range count) of one layer; waits for the pending accumulates."""
        cc = self.forest_info()["class_counts"]
        Cn = cc[layer] if 0 <= layer < len(cc) else 1   # a layer the model does not have: the library refuses it
        counts = np.empty((Cn, Cn), np.uint64)
        oor = C.c_uint64()
        capi.check(self.h, self.L.rvseg_eval_confusion(self.h, layer, _ptr(counts), C.byref(oor)))
        return counts, oor.value

    def debug_lattice_builds(self):
        """Lattices built on this context so far (overflow retries included): a call that must build none leaves it unchanged."""
        n = C.c_longlong()
        capi.check(self.h, self.L.rvseg_debug_lattice_builds(self.h, C.byref(n)))
        return n.value

    def last_timing(self):
        names = C.create_string_buffer(4096)
        ms = (C.c_float * 64)()
        n = self.L.rvseg_last_timing(self.h, names, 4096, ms, 64)
        ns = names.value.decode().split(";") if names.value else []
        return {ns[i]: ms[i] for i in range(min(n, len(ns)))}


# ---------------------------------------------------------------------------------------------
# reference-shaped facades
# ---------------------------------------------------------------------------------------------
class RandomForest:
    """libf::RandomForest as the hot path uses it (classifiers.h:274-344)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def read(self, src):  # RandomForest::read(std::istream&), classifier.cpp:222
        self.ctx.forest_load(src)

    def write(self, dst=None):  # RandomForest::write(std::ostream&), classifier.cpp:210
        return self.ctx.forest_write(dst)

    def getSize(self):
        return self.ctx.forest_info()["n_trees"]

    def classLogPosterior(self, X):  # classifier.cpp:166 -- ctx must have multi_layer=0
        return self.ctx.forest_eval(np.atleast_2d(X))

    def multiClassLogPosterior(self, X):  # classifier.cpp:187 -- ctx must have multi_layer=1
        out = self.ctx.forest_eval(np.atleast_2d(X))
        cc = self.ctx.forest_info()["class_counts"]
        offs = np.cumsum([0] + cc)
        return [out[:, offs[i]:offs[i + 1]] for i in range(len(cc))]

    def classify(self, X, layer=0):  # Classifier::classify(DataStorage), classifier.cpp:29-62, on the device
        return self.ctx.forest_classify(np.atleast_2d(X), layer)

    def updateHistograms(self, X, labels, class_counts, smoothing=1.0):
        """DecisionTreeLearner::updateHistograms / updateMultiHistograms (learning.cpp:918-1012) on every tree: returns
        the forest.dat bytes of the same trees with their leaves re-estimated; read() them to use them."""
        return self.ctx.forest_refit(X, labels, class_counts, smoothing)


class BoostedRandomForest:
    """libf::BoostedRandomForest (classifiers.h:349-425) on a context with multi_layer=0."""

    def __init__(self, ctx):
        self.ctx = ctx

    def read(self, src, order=capi.BOOSTED_WEIGHT_FIRST):  # BoostedRandomForest::read, classifier.cpp:264 (order: see Context.boosted_load)
        self.ctx.boosted_load(src, order)

    def write(self, dst=None, order=capi.BOOSTED_AS_LOADED):  # BoostedRandomForest::write, classifier.cpp:250
        return self.ctx.boosted_write(dst, order)

    def getSize(self):
        return int(self.ctx.boosted_weights().size)

    def getWeights(self):
        return self.ctx.boosted_weights()

    def classLogPosterior(self, X):  # classifier.cpp:283-302: the weighted votes per class
        return self.ctx.forest_eval(np.atleast_2d(X))

    def classify(self, X):  # Classifier::classify, classifier.cpp:29-51: the first strictly greatest vote sum
        post = self.classLogPosterior(X)
        label = np.zeros(post.shape[0], np.int32)
        best = post[:, 0].copy()
        for c in range(1, post.shape[1]):
            win = post[:, c] > best
            label[win] = c
            best[win] = post[win, c]
        return label


# libforest tools.h: `classifier` / `forest` is a RandomForest or BoostedRandomForest wrapper; X (P, D), labels (P,).  The
# counts come from the device in one pass (Context.forest_measure), the floats from the reference's arithmetic on them.
class AccuracyTool:
    """libf::AccuracyTool (tools.cpp:61-89)."""

    def measure(self, classifier, X, labels, layer=0):
        return capi.forest_tools_scores(classifier.ctx.forest_measure(np.atleast_2d(X), labels, layer, want=("confusion",))["confusion"])[0]

    def format(self, accuracy):
        return "Accuracy: %2.2f%% (Error: %2.2f%%)\n" % (accuracy * 100, (1 - accuracy) * 100)

    def print(self, accuracy):
        print(self.format(accuracy), end="")

    def measureAndPrint(self, classifier, X, labels, layer=0):
        self.print(self.measure(classifier, X, labels, layer))


class ConfusionMatrixTool:
    """libf::ConfusionMatrixTool (tools.cpp:95-186): rows are true classes, a class without examples is a NaN row."""

    def measure(self, classifier, X, labels, layer=0):
        return capi.forest_tools_scores(classifier.ctx.forest_measure(np.atleast_2d(X), labels, layer, want=("confusion",))["confusion"])[1]

    def format(self, result):  # tools.cpp:140-179 without the colour codes
        n = len(result)
        rule = "--------|" * (n + 1) + "\n"
        out = "        |" + "".join(" %6d |" % c for c in range(n)) + "\n" + rule
        for c in range(n):
            out += " %6d |" % c + "".join(" %5.2f%% |" % (result[c][cc] * 100) for cc in range(n)) + "\n" + rule
        return out

    def print(self, result):
        print(self.format(result), end="")

    def measureAndPrint(self, classifier, X, labels, layer=0):
        self.print(self.measure(classifier, X, labels, layer))


class CorrelationTool:
    """libf::CorrelationTool (tools.cpp:192-263): per tree pair, 1 - the normalised Hamming distance of their votes."""

    def measure(self, forest, X, layer=0):
        X = np.atleast_2d(X)
        return capi.forest_tools_correlation(forest.ctx.forest_measure(X, None, layer, want=("agree",))["agree"], X.shape[0])

    def format(self, result):  # tools.cpp:233-263
        n = len(result)
        rule = "---------|" * (n + 1) + "\n"
        out = "         |" + "".join(" %7d |" % c for c in range(n)) + "\n" + rule
        for c in range(n):
            out += " %7d |" % c + "".join(" %6.2f%% |" % (result[c][cc] * 100) for cc in range(n)) + "\n" + rule
        return out

    def print(self, result):
        print(self.format(result), end="")

    def measureAndPrint(self, forest, X, layer=0):
        self.print(self.measure(forest, X, layer))


class RandomForestPrune:
    """libf::RandomForestPrune (todos.txt:12-18, 310-350): simulated annealing over the trees of a forest.  The settings
    are rvseg_prune_params' (the reference's schedule, the exchange move and the error energy by default); `trace` holds
    the rows of the last run, which format() prints the way PruneCallback does."""

    def __init__(self, **params):
        self.params = params
        self.trace = None
        self.state = None

    def prune(self, forest, X, labels, layer=0, state=None):
        """Prunes forest (a RandomForest wrapper) on (X, labels): its context's model becomes the forest of the best
        state's trees (todos.txt:343-349), which forest.write() then emits.  Returns forest."""
        run = forest.ctx.forest_prune(np.atleast_2d(X), labels, layer, state, **self.params)
        self.trace, self.state = run["trace"], run["state"]
        forest.ctx.forest_prune_apply(run["state"])
        return forest

    def format(self, trace=None):  # PruneCallback::callback, todos.txt:36-41
        rows = self.trace if trace is None else trace
        return "".join("iteration: %d energy: %g best: %g temp: %g state: %d\n" % (r["iteration"], r["energy"], r["best_energy"], r["temperature"],
                                                                                r["state_size"]) for r in rows)


class FeatureExtractor:
    """Features::FeatureExtractor (include/feature_extractor.h:24-41), NO_LABEL extraction."""

    def __init__(self, ctx):
        self.ctx = ctx

    def extract(self, color, depth, calib):
        return self.ctx.extract_features(color, depth, calib)


CONST_KERNEL, DIAG_KERNEL, FULL_KERNEL = capi.CONST_KERNEL, capi.DIAG_KERNEL, capi.FULL_KERNEL
NO_NORMALIZATION, NORMALIZE_BEFORE, NORMALIZE_AFTER, NORMALIZE_SYMMETRIC = (
    capi.NO_NORMALIZATION, capi.NORMALIZE_BEFORE, capi.NORMALIZE_AFTER, capi.NORMALIZE_SYMMETRIC)


class PottsCompatibility:
    """out = -w * Q (labelcompatibility.cpp:43-55); parameters: [w]."""
    kind = capi.COMPAT_POTTS

    def __init__(self, weight):
        self.w = np.float32(weight)

    def parameters(self):
        return np.array([self.w], np.float32)

    def setParameters(self, v):
        self.w = np.float32(v[0])

    def array(self, M):
        return np.array([self.w], np.float32)



class DiagonalCompatibility:
    """out = diag(v) * Q (labelcompatibility.cpp:61-73); parameters: v."""
    kind = capi.COMPAT_DIAGONAL

    def __init__(self, v):
        self.v = np.array(v, np.float32).reshape(-1)

    def parameters(self):
        return self.v.copy()

    def setParameters(self, v):
        self.v = np.array(v, np.float32).reshape(-1)

    def array(self, M):
        assert self.v.shape == (M,)
        return self.v


class MatrixCompatibility:
    """out = W * Q with W = 0.5 (m + m^T) in fp32 (labelcompatibility.cpp:79-100); parameters: the upper triangle of W
    row by row (W[i][j], j >= i), as parameters() / setParameters() pack it (:88-100)."""
    kind = capi.COMPAT_MATRIX

    def __init__(self, m):
        m = np.array(m, np.float32)
        assert m.ndim == 2 and m.shape[0] == m.shape[1]
        self.W = np.float32(0.5) * (m + m.T)

    def parameters(self):
        M = self.W.shape[0]
        return np.array([self.W[i, j] for i in range(M) for j in range(i, M)], np.float32)

    def setParameters(self, v):
        M = self.W.shape[0]
        v = np.asarray(v, np.float32)
        assert v.shape == (M * (M + 1) // 2,)
        k = 0
        for i in range(M):
            for j in range(i, M):
                self.W[i, j] = self.W[j, i] = v[k]
                k += 1

    def array(self, M):
        assert self.W.shape == (M, M)
        return np.ascontiguousarray(self.W)   # symmetric: the library's 0.5 (W + W^T) is W again


def _compat(c):
    return c if hasattr(c, "kind") else PottsCompatibility(c)


def _crf_terms(terms, M, N, device=False):
    """ctypes rvseg_crf_term array for [(features, compatibility, kernel_type, normalization, kernel_params)]; the second
    value keeps the numpy buffers alive for the call."""
    arr = (capi.RvsegCrfTerm * max(1, len(terms)))()
    keep = []
    for k, (f, comp, kt, nt, kp) in enumerate(terms):
        comp = _compat(comp)
        cp = np.ascontiguousarray(comp.array(M), np.float32)
        keep.append(cp)
        t = arr[k]
        if device:
            t.d, t.features = int(f[1]), C.c_void_p(f[0])   # (device address, d)
        else:
            fa = np.ascontiguousarray(f, np.float32)
            assert fa.shape[0] == N
            keep.append(fa)
            t.d, t.features = fa.shape[1], fa.ctypes.data
        t.compat, t.kernel_type, t.normalization = comp.kind, int(kt), int(nt)
        t.compat_params = cp.ctypes.data
        if kp is not None and int(kt) != CONST_KERNEL:
            kpa = np.ascontiguousarray(kp, np.float32).reshape(-1)
            assert kpa.shape == ((t.d if int(kt) == DIAG_KERNEL else t.d * t.d),)
            keep.append(kpa)
            t.kernel_params = kpa.ctypes.data
    return arr, keep


class _Objective:
    """An ObjectiveFunction of objective.h over ground-truth labels gt (N, int16; a label outside 0 .. C-1 skips its point)."""
    kind = None

    def __init__(self, gt):
        self.gt = np.ascontiguousarray(gt, np.int16).reshape(-1)
        self.robust = 0.0

    def weights(self, M):
        return None

    def record(self, N, M, d_gt=0, d_class_weight=0):
        """(rvseg_crf_objective, buffers to keep alive).  d_gt / d_class_weight: device addresses for the _device entries."""
        assert self.gt.shape == (N,)
        w = self.weights(M)
        rec = capi.RvsegCrfObjective(self.kind, d_gt or self.gt.ctypes.data, float(self.robust),
                                     d_class_weight or (w.ctypes.data if w is not None else None))
        return rec, (self.gt, w)


class LogLikelihood(_Objective):   # objective.cpp:35-50
    kind = capi.OBJECTIVE_LOGLIKELIHOOD

    def __init__(self, gt, robust=0.0):
        super().__init__(gt)
        self.robust = float(robust)


class Hamming(_Objective):   # objective.cpp:51-79
    """Hamming(gt, class_weight_pow) computes the class weights on the host as the reference's constructor does (:51-63,
    fp32); Hamming(gt, weights) takes them."""
    kind = capi.OBJECTIVE_HAMMING

    def __init__(self, gt, class_weight_pow=0.0):
        super().__init__(gt)
        if np.ndim(class_weight_pow) > 0:
            self.class_weight = np.array(class_weight_pow, np.float32).reshape(-1)
            return
        M = max(0, int(self.gt.max()) + 1) if self.gt.size else 0
        cnt = np.bincount(self.gt[self.gt >= 0].astype(np.int64), minlength=M).astype(np.float32)
        with np.errstate(all="ignore"):
            w = cnt / cnt.sum(dtype=np.float32)
            w = np.power(w, np.float32(-float(class_weight_pow))).astype(np.float32)
            self.class_weight = (w / (cnt * w).sum(dtype=np.float32)).astype(np.float32)

    def weights(self, M):
        w = np.zeros(M, np.float32)   # one weight per class of the model; classes beyond the given ones weigh 0
        n = min(M, self.class_weight.shape[0])
        w[:n] = self.class_weight[:n]
        return w


class IntersectionOverUnion(_Objective):   # objective.cpp:80-108
    kind = capi.OBJECTIVE_IOU


class DenseCRF:
    """DenseCRF as Segmenter::processMapFromQueue drives it (src/segmenter.cpp:641-644), and as
    examples/dense_learning.cpp:128-182 builds a learned model (compatibilities, kernel types and parameters,
    normalisations, a logistic unary)."""

    def __init__(self, ctx, N, M):
        self.ctx, self.N, self.M = ctx, N, M
        self.unary = None
        self.logistic = None    # (L: M x K, f: N x K) of setUnaryEnergy(L, f)
        # per term: [features, compatibility (float = Potts), kernel_type, normalization, kernel parameters or None]
        self.kernels = []

    def setUnaryEnergy(self, unary, f=None):  # densecrf.cpp:85-91; unary is N x M energy (= -log-posterior)
        if f is not None:   # setUnaryEnergy(L, f): LogisticUnaryEnergy, unary.cpp:44-52 (L: M x K, f: N x K point-major)
            L = np.array(unary, np.float32)
            f = np.ascontiguousarray(f, np.float32)
            assert L.shape[0] == self.M and f.shape == (self.N, L.shape[1])
            self.logistic, self.unary = (L, f), None
            self._update_model(lambda: self.ctx.crf_model_set_logistic(L, f))   # the live model keeps f
            return
        self._touch()
        unary = np.ascontiguousarray(unary, np.float32)
        assert unary.shape == (self.N, self.M)
        self.unary, self.logistic = unary, None

    def addPairwiseEnergy(self, features, function, kernel_type=DIAG_KERNEL, normalization=NORMALIZE_SYMMETRIC):  # densecrf.cpp:54-60
        features = np.ascontiguousarray(features, np.float32)
        assert features.shape[0] == self.N  # assert(features.cols() == N_), densecrf.cpp:55
        self._touch()
        if not hasattr(function, "kind"):
            function = float(function)   # a bare weight: PottsCompatibility(w)
        self.kernels.append([features, function, int(kernel_type), int(normalization), None])

    def addPairwiseGaussian(self, W, H, sx, sy, w, kernel_type=DIAG_KERNEL, normalization=NORMALIZE_SYMMETRIC):  # densecrf.cpp:61-69
        self.addPairwiseEnergy(capi.crf_features_gaussian(W, H, sx, sy), w, kernel_type, normalization)

    def addPairwiseBilateral(self, W, H, sx, sy, sr, sg, sb, im, w, kernel_type=DIAG_KERNEL,
                             normalization=NORMALIZE_SYMMETRIC):  # densecrf.cpp:70-81
        self.addPairwiseEnergy(capi.crf_features_bilateral(W, H, sx, sy, sr, sg, sb, im), w, kernel_type, normalization)

    # ---- parameters (densecrf.cpp:294-360) ----
    def unaryParameters(self):   # LogisticUnaryEnergy::parameters, unary.cpp:53-57: L column-major
        if self.logistic is None:
            return np.zeros(0, np.float32)
        return np.ascontiguousarray(self.logistic[0].T).reshape(-1)

    def _assign_unary(self, v):   # this object's copy only, as the other _assign_*: no model call
        L, f = self.logistic
        v = np.asarray(v, np.float32)
        assert v.shape == (L.size,)
        self.logistic = (np.ascontiguousarray(v.reshape(L.shape[1], L.shape[0]).T), f)

    def setUnaryParameters(self, v):   # unary.cpp:58-63
        if self.logistic is None:
            return
        self._assign_unary(v)
        self._update_model(lambda: self.ctx.crf_model_set_logistic_params(self.logistic[0]))   # U = L f again from the kept f

    def labelCompatibilityParameters(self):
        return np.concatenate([np.zeros(0, np.float32)] + [_compat(k[1]).parameters() for k in self.kernels]).astype(np.float32)

    def _assign_compat(self, v):
        v = np.asarray(v, np.float32)
        i = 0
        for k in self.kernels:
            k[1] = _compat(k[1])
            n = k[1].parameters().shape[0]
            k[1].setParameters(v[i:i + n])
            i += n
        assert i == v.shape[0]

    def setLabelCompatibilityParameters(self, v):
        self._assign_compat(v)

        def update():
            for t, k in enumerate(self.kernels):
                self.ctx.crf_model_set_compat(t, k[1])
        self._update_model(update)

    def _kernel_parameters(self, k):   # DenseKernel::parameters, pairwise.cpp:116-125
        d = k[0].shape[1]
        if k[2] == CONST_KERNEL:
            return np.zeros(0, np.float32)
        if k[4] is not None:
            return k[4].copy()
        return np.ones(d, np.float32) if k[2] == DIAG_KERNEL else np.eye(d, dtype=np.float32).reshape(-1)

    def kernelParameters(self):
        return np.concatenate([np.zeros(0, np.float32)] + [self._kernel_parameters(k) for k in self.kernels]).astype(np.float32)

    def _assign_kernel(self, v):
        """Returns the terms whose values changed: those whose lattice a live model has to build again."""
        v = np.asarray(v, np.float32)
        i = 0
        changed = []
        for t, k in enumerate(self.kernels):
            n = self._kernel_parameters(k).shape[0]
            if k[2] != CONST_KERNEL:
                new = v[i:i + n].copy()
                if k[4] is None or k[4].tobytes() != new.tobytes():
                    changed.append(t)
                k[4] = new
            i += n
        assert i == v.shape[0]
        return changed

    def setKernelParameters(self, v):   # pairwise.cpp:140-152: DIAG d values, FULL d x d column-major, CONST none
        changed = self._assign_kernel(v)

        def update():
            for t in changed:
                self.ctx.crf_model_set_kernel(t, self.kernels[t][4])
        self._update_model(update)

    def _unary_energy(self):
        # A logistic unary is computed on the GPU and read back, then uploaded with the model (an N x M round trip per
        # inference); device-resident callers use Context.crf_logistic_unary_device + crf_infer_terms_device instead.
        if self.logistic is not None:
            return self.ctx.crf_logistic_unary(*self.logistic)
        return self.unary if self.unary is not None else np.zeros((self.N, self.M), np.float32)

    def inference(self, n_iterations, label_mode=capi.LABEL_ARGMAX, unknown_label=0):  # densecrf.cpp:115-131
        U = self._unary_energy()
        plain = all(isinstance(k[1], float) and k[3] == NORMALIZE_SYMMETRIC and k[4] is None for k in self.kernels)
        if not plain:
            return self.ctx.crf_infer_terms(U, [tuple(k) for k in self.kernels], n_iterations, label_mode, unknown_label)
        if len(self.kernels) == 1:
            f, w = self.kernels[0][:2]
            return self.ctx.crf_infer(U, f, w, n_iterations, label_mode, unknown_label)
        return self.ctx.crf_infer_multi(U, [k[0] for k in self.kernels], [k[1] for k in self.kernels], n_iterations, label_mode, unknown_label)

    def map(self, n_iterations):  # densecrf.cpp:132-137
        return self.inference(n_iterations, capi.LABEL_ARGMAX)[1]

    # ---- stepwise inference, energies, KL divergence (densecrf.h:77-94) on a model the context keeps ----
    # The context has one model and no handle for it: objects that share a context take turns, and anybody may set a model
    # on it directly.  _model_serial is the serial crf_model_set returned for this object's model (0: none, or changed since).
    def _touch(self):
        self._model_serial = 0

    def _model_is_live(self):
        serial = getattr(self, "_model_serial", 0)
        return serial != 0 and self.ctx.crf_model_serial() == serial

    def _update_model(self, update):
        """A parameter change: in place on the context's live model when that model is this object's (no lattice build),
        else the model is set again by the next call that needs it."""
        if self._model_is_live():
            update()
        else:
            self._touch()

    def _with_model(self, call):
        """Runs call() on this CRF's model: set lazily, again after any add* / set*Parameters, and again when the context
        keeps another model or none."""
        if not self._model_is_live():
            self._touch()   # (a failure below leaves no model of this object)
            if self.logistic is not None:   # the model computes L f itself and keeps f
                serial = self.ctx.crf_model_set(np.zeros((self.N, self.M), np.float32), [tuple(k) for k in self.kernels])
                self.ctx.crf_model_set_logistic(*self.logistic)
            else:
                serial = self.ctx.crf_model_set(self._unary_energy(), [tuple(k) for k in self.kernels])
            self._model_serial = serial
        return call()

    def startInference(self):  # densecrf.cpp:178-186
        return self._with_model(self.ctx.crf_model_start)

    def stepInference(self, Q, n_steps=1):  # densecrf.cpp:187-201; returns the stepped copy
        return self._with_model(lambda: self.ctx.crf_model_step(Q, n_steps))

    def currentMap(self, Q):  # densecrf.cpp:202-211
        return self.ctx.label_values(np.ascontiguousarray(Q, np.float32), capi.LABEL_ARGMAX)

    def unaryEnergy(self, l):  # densecrf.cpp:141-153
        return self._with_model(lambda: self.ctx.crf_model_energy(l, -1, True, False))[0]

    def pairwiseEnergy(self, l, term=-1):  # densecrf.cpp:154-177
        return self._with_model(lambda: self.ctx.crf_model_energy(l, term, False, True))[1]

    def klDivergence(self, Q, parts=False):  # densecrf.cpp:214-235; parts: (kl, [entropy, unary, term 0, ...])
        p = self._with_model(lambda: self.ctx.crf_model_kl(Q))
        kl = 0.0
        for v in p:
            kl += float(v)
        return (kl, p) if parts else kl

    def inference_trace(self, n_iterations):
        """(Q, kl): inference(n) and the KL divergence after the start and after every iteration."""
        Q, _, kl = self._with_model(lambda: self.ctx.crf_model_trace(n_iterations))
        return Q, kl

    # ---- learning (densecrf.cpp:238-297) ----
    def applyTranspose(self, term, Q):   # pairwise.cpp:179-183
        return self._with_model(lambda: self.ctx.crf_model_apply_transpose(term, Q))

    def kernelGradient(self, term, b, Q):   # pairwise.cpp:202-207: kernel_->gradient(b, compatibility(Q)), fp32
        return self._with_model(lambda: self.ctx.crf_model_kernel_gradient(term, b, self.ctx.crf_model_compat_apply(term, Q))).astype(np.float32)

    def gradient(self, n_iterations, objective, unary=True, lbl_cmp=True, energy_grad=False, kernel=False):
        """DenseCRF::gradient: (value, unary_grad, lbl_cmp_grad) in fp32 with the reference's signs and layouts: unary_grad
        is the gradient of unaryParameters() (empty without a logistic unary), lbl_cmp_grad that of
        labelCompatibilityParameters(); a part not asked for is None.  kernel: a fourth element, the gradient of
        kernelParameters().  energy_grad: unary_grad is d value / d U (N x M) instead."""
        if self.logistic is not None and unary and not energy_grad:   # one call; C K doubles come back, not N x M floats
            value, ug, cg, kg = self._with_model(lambda: self.ctx.crf_model_gradient_params(n_iterations, objective, True, lbl_cmp, kernel))
        elif kernel:
            value, ug, cg, kg, _ = self._with_model(lambda: self.ctx.crf_model_gradient_kernel(n_iterations, objective, unary, lbl_cmp))
        else:
            value, ug, cg, _ = self._with_model(lambda: self.ctx.crf_model_gradient(n_iterations, objective, unary, lbl_cmp))
        if unary and not energy_grad:   # of unaryParameters(): none without a logistic unary
            ug = np.zeros(0, np.float32) if self.logistic is None else ug.astype(np.float32)
        out = (value, ug, (cg.astype(np.float32) if lbl_cmp else None))
        return out + (kg.astype(np.float32),) if kernel else out

    def energy_gradient(self, n_iterations, objective, unary, pairwise, kernel, l2_norm, x):
        """CRFEnergy::gradient (dense_learning.cpp:60-84) as one rvseg_crf_model_energy_gradient: x becomes this object's
        parameters and the live model's; (value, dx)."""
        x = np.asarray(x, np.float32)
        nu = self.unaryParameters().shape[0] if unary else 0
        nc = self.labelCompatibilityParameters().shape[0] if pairwise else 0
        nk = self.kernelParameters().shape[0] if kernel else 0
        assert x.shape == (nu + nc + nk,)
        mask = (capi.LEARN_UNARY if unary else 0) | (capi.LEARN_PAIRWISE if pairwise else 0) | (capi.LEARN_KERNEL if kernel else 0)
        try:
            if nu:
                self._assign_unary(x[:nu])
            if pairwise:
                self._assign_compat(x[nu:nu + nc])
            if kernel:
                self._assign_kernel(x[nu + nc:])
            return self._with_model(lambda: self.ctx.crf_model_energy_gradient(n_iterations, objective, mask, l2_norm, x))
        except BaseException:
            self._touch()   # the model may hold a part of x only: the next call sets it afresh
            raise


class CRFEnergy:
    """The EnergyFunction of examples/dense_learning.cpp:38-85 over a DenseCRF: gradient(x) sets the parameters, and returns
    the negated objective and gradient plus the L2 term (one rvseg_crf_model_energy_gradient on the kept model), for
    minimizeLBFGS.  Unary and label-compatibility parameters only: CRFKernelEnergy also learns the kernel parameters."""

    def __init__(self, crf, objective, NIT, unary=True, pairwise=True, kernel=False):
        if kernel:
            raise NotImplementedError("CRFEnergy(kernel=True): this class learns unary and pairwise parameters only; use "
                                      "CRFKernelEnergy for the kernel parameters as well")
        self.crf, self.objective, self.NIT = crf, objective, int(NIT)
        self.unary, self.pairwise = bool(unary), bool(pairwise)
        self.initial_u_param = crf.unaryParameters()
        self.initial_lbl_param = crf.labelCompatibilityParameters()
        self.l2_norm = np.float32(0.0)
        # the parameter groups of x in order: (learned?, initial value, setter); a subclass appends its own
        self.groups = [(self.unary, self.initial_u_param, crf.setUnaryParameters),
                       (self.pairwise, self.initial_lbl_param, crf.setLabelCompatibilityParameters)]

    def _crf_gradient(self):
        """(value, [one gradient per group, None where the group is not learned])."""
        r, du, dl = self.crf.gradient(self.NIT, self.objective, self.unary, self.pairwise)
        return r, [du, dl]

    def setL2Norm(self, norm):
        self.l2_norm = np.float32(norm)

    def initialValue(self):
        return np.concatenate([np.zeros(0, np.float32)] + [p for on, p, _ in self.groups if on]).astype(np.float32)

    def gradient(self, x):
        """(value, dx) of dense_learning.cpp:60-84: one rvseg_crf_model_energy_gradient on the kept model of a DenseCRF (its
        definition in rvseg.h: the L2 term of the value is summed in double)."""
        x = np.asarray(x, np.float32)
        assert x.shape == (sum(p.shape[0] for on, p, _ in self.groups if on),)
        if not hasattr(getattr(self.crf, "ctx", None), "crf_model_energy_gradient"):
            return self._compose(x)
        return self.crf.energy_gradient(self.NIT, self.objective, self.unary, self.pairwise, getattr(self, "kernel", False), self.l2_norm, x)

    def _compose(self, x):
        """gradient(x) over any object with DenseCRF's setters and gradient(), call by call.  dx as the one entry gives it; the
        L2 term of the value is 0.5 l2 x.x with the dot product in fp32."""
        i = 0
        for on, p, setter in self.groups:
            if on:
                setter(x[i:i + p.shape[0]])
                i += p.shape[0]
        r, grads = self._crf_gradient()
        dx = np.concatenate([np.zeros(0, np.float32)] + [-g for (on, _, _), g in zip(self.groups, grads) if on]).astype(np.float32)
        r = -r
        if self.l2_norm > 0:
            dx = (dx + self.l2_norm * x).astype(np.float32)
            r += 0.5 * float(self.l2_norm) * float(np.dot(x, x))
        return r, dx


class CRFKernelEnergy(CRFEnergy):
    """The whole EnergyFunction of examples/dense_learning.cpp:38-85: CRFEnergy with the kernel parameters as the third
    group of x.  A gradient(x) with kernel=True builds again only the lattices of the terms whose parameters changed, from
    the features the model keeps."""

    def __init__(self, crf, objective, NIT, unary=True, pairwise=True, kernel=True):
        CRFEnergy.__init__(self, crf, objective, NIT, unary, pairwise, False)
        self.kernel = bool(kernel)
        self.initial_knl_param = crf.kernelParameters()
        self.groups.append((self.kernel, self.initial_knl_param, crf.setKernelParameters))

    def _crf_gradient(self):
        g = self.crf.gradient(self.NIT, self.objective, self.unary, self.pairwise, kernel=self.kernel)
        return g[0], [g[1], g[2], g[3] if self.kernel else None]


def minimizeLBFGS(energy, restart=0, verbose=False, report=None, **params):
    """minimizeLBFGS of optimization.cpp:68-103 on rvseg_minimize_lbfgs: epsilon = 1e-6 and max_iterations = 50 unless given
    in params (fields of rvseg_lbfgs_params), up to restart + 1 runs from where the last one ended, stopping when a run's
    value is no lower than the lowest before it.  energy: initialValue() and gradient(x float32) -> (value, dx), as
    CRFEnergy.  x crosses to the energy as float32 (the reference's VectorXf).  Returns the parameters, float32.
    report (optional list): one dict per run, capi.minimize_lbfgs's with "fx"."""
    x = np.array(energy.initialValue(), np.float64).reshape(-1)
    if x.shape[0] == 0:
        return x.astype(np.float32)
    p = dict(epsilon=1e-6, max_iterations=50)
    p.update(params)

    def fun(xd):
        value, dx = energy.gradient(xd.astype(np.float32))
        return value, np.asarray(dx, np.float64)

    def progress(xd, g, fx, xnorm, gnorm, step, k, ls):
        print("Iteration %d:\n  fx = %f, xnorm = %f, gnorm = %f, step = %f\n" % (k, fx, xnorm, gnorm, step))
        return 0

    last_f = 1e100
    rep = {}
    for _ in range(int(restart) + 1):
        x, fx, rep = capi.minimize_lbfgs(fun, x, progress if verbose else None, **p)
        if report is not None:
            report.append(dict(rep, fx=fx))
        if last_f > fx:
            last_f = fx
        else:
            break
    if verbose:
        print("L-BFGS optimization terminated with status code = %d" % rep.get("status", 0))
    return x.astype(np.float32)


def numericGradient(energy, x, EPS=1e-3):   # optimization.cpp:104-115
    x = np.asarray(x, np.float32)
    g = np.empty(x.shape[0], np.float32)
    for i in range(x.shape[0]):
        xx = x.copy()
        xx[i] = x[i] + np.float32(EPS)
        v1 = energy.gradient(xx)[0]
        xx[i] = x[i] - np.float32(EPS)
        v0 = energy.gradient(xx)[0]
        g[i] = (v1 - v0) / (2 * EPS)
    return g


def gradCheck(energy, x, EPS=1e-3):   # optimization.cpp:121-126: the norm of numeric minus analytic gradient
    ng = numericGradient(energy, x, EPS)
    g = np.asarray(energy.gradient(np.asarray(x, np.float32))[1], np.float32)
    return float(np.linalg.norm((ng - g).astype(np.float32)))


class LocalMapStore:
    """_cloud_results plus the two services that read it (src/segmenter.cpp:711-774): (map id,
    result_labels[layer]) pairs in arrival order.  Host only."""

    def __init__(self, layer_names):
        self.layer_names = list(layer_names)
        self.results = []

    def store(self, local_map_id, result_labels):  # :711-713
        self.results.append((int(local_map_id), [np.asarray(l, np.uint8).copy() for l in result_labels]))

    def srvStoredSemanticsIds(self):  # :722-729 -> IdsSrv response `int32[] local_map_ids`
        return [m[0] for m in self.results]

    def srvGetLocalMapSegmentation(self, local_map_id, segmentation_layers):
        """:731-774 -> (local_map_id, uint8[] point_labels = requested layers concatenated) or False for an
        unknown layer name (:744-746) or map id (:773)."""
        idx = []
        for name in segmentation_layers:
            if name in self.layer_names:
                idx.append(self.layer_names.index(name))
        if len(idx) != len(segmentation_layers):
            return False
        for mid, labels in self.results:
            if mid == local_map_id:
                parts = [labels[l] for l in idx]
                return mid, (np.concatenate(parts) if parts else np.zeros(0, np.uint8))
        return False


class Segmenter:
    """The per-frame inference part of `class Segmenter` (include/segmenter.h:47-69), ROS-free:
    construction loads the forest like Segmenter::Segmenter (src/segmenter.cpp:106-129),
    processFrames does what processFramesFromQueueInternalRF does per dequeued frame
    (src/segmenter.cpp:351-431) for a whole batch, plus the per-frame DenseCRF when enabled;
    processMap is processMapFromQueue for one local map; the srv* methods are the three services
    (:722-792) over plain Python values.

    layers (optional): [{"name": str, "classes": [(class name, (r, g, b)), ...]}, ...] -- the
    `color_codings` of config.json (:73-98); needed only by the services and the cloud dumps.

    external_semantics=True selects the other single-frame provider (launch/semantics.launch; :101-103, 227-228):
    forest may be None, `layers` gives the layout (as single_frame_segmentation_server.py:68-71 reads it from the
    config), and processFrames takes the provider's label_distribution -- or a provider callable -- instead of running
    the forest (processFramesFromQueueExternal, :445-514)."""

    def __init__(self, forest, layers=None, external_semantics=False, **params):
        self.external_semantics = bool(external_semantics)
        if self.external_semantics and layers is None:
            raise RuntimeError("external_semantics needs the label layers (the layout comes from the config, not from a model)")
        self.ctx = Context(**params)
        if forest is not None:
            self.ctx.forest_load(forest)
        elif not self.external_semantics:
            self.ctx.close()
            raise RuntimeError("no forest given (only external_semantics runs without one)")
        if self.external_semantics:
            self.layer_class_counts = [len(l["classes"]) for l in layers]
            try:
                self.ctx.external_layers_set(self.layer_class_counts)
            except capi.RvsegError:
                self.ctx.close()
                raise
        else:
            self.layer_class_counts = self.ctx.forest_info()["class_counts"]
        self.layer_count = len(self.layer_class_counts)
        if layers is None:
            layers = [{"name": "layer%d" % l, "classes": [("class%d" % c, (0, 0, 0)) for c in range(n)]}
                      for l, n in enumerate(self.layer_class_counts)]
        if [len(l["classes"]) for l in layers] != list(self.layer_class_counts):
            self.ctx.close()
            raise RuntimeError("model / config mismatch: layer or class counts (README.md:30 of the reference)")
        self.layers = layers
        self.store = LocalMapStore([l["name"] for l in layers])

    def processFrames(self, color, depth, calib, label_distribution=None, provider=None, dist_stride=1, **kw):
        """Internal forest: segment_frames.  With external_semantics: label_distribution (n, S * h * w), or `provider`,
        a callable taking the request of externalRequest() and returning it; a provider that fails raises, as the
        reference throws when the service call fails (:505)."""
        if not self.external_semantics:
            if label_distribution is not None or provider is not None:
                raise RuntimeError("label_distribution / provider need external_semantics=True")
            return self.ctx.segment_frames(color, depth, calib, **kw)
        if label_distribution is None:
            if provider is None:
                raise RuntimeError("external_semantics: pass label_distribution or a provider")
            try:
                label_distribution = provider(self.externalRequest(color, depth, calib))
            except Exception as e:
                raise RuntimeError("Calling the segmentation service failed!") from e
        return self.ctx.segment_external(color, depth, calib, label_distribution, dist_stride, **kw)

    def externalRequest(self, color, depth, calib):
        """The SingleFrameSegmentation request of :490-502 for a batch: {"rgb": (n, H, W, 3) uint8 (RGB8),
        "depth": (n, H, W, 3) float32 (TYPE_32FC3, the rectified xyz image; NaN outside 0.5 .. 15 m, :472)}."""
        return {"rgb": np.ascontiguousarray(color, np.uint8), "depth": self.ctx.rectify_depth(depth, calib, 0.5, 15.0)}

    def processMap(self, index_images=None, posteriors=None, cloud_xyz=None, cloud_rgb=None, unknown_labels=None, local_map_id=None,
                   projections=None):
        """The body of processMapFromQueue for one local map (src/segmenter.cpp:561-682): fuse the frames'
        label distributions into per-point unaries through the index images, then per layer either the
        cloud DenseCRF with the thresholded argmax (:628-658) or the no-CRF rule (:660-681).
        cloud_rgb is in [0, 1] like fps_mapper's cloud (:698-700).  With local_map_id the labels are kept
        for the services (:711-713).  Returns (result_labels, unaries).
        projections=P (n_images x 3 x 4) instead of index_images=: the projector makes the index images from one
        projection matrix per sub-image (:576-578; Context.project_cloud)."""
        if (index_images is None) == (projections is None):
            raise RuntimeError("processMap takes either index_images or projections")
        if posteriors is None or cloud_xyz is None or cloud_rgb is None:
            raise RuntimeError("processMap needs posteriors, cloud_xyz and cloud_rgb")
        p = self.ctx.params
        cc = self.layer_class_counts
        # the layout comes from the context's model: none (a refused load raises ERR_NO_FOREST here) or another one
        if not self.external_semantics and self.ctx.forest_info()["class_counts"] != list(cc):
            raise RuntimeError("model / config mismatch: layer or class counts (README.md:30 of the reference)")
        cloud_xyz = np.ascontiguousarray(cloud_xyz, np.float32)
        cloud_rgb = np.ascontiguousarray(cloud_rgb, np.float32)
        n_pts = cloud_xyz.shape[0]
        if projections is not None:
            index_images = self.ctx.project_cloud(projections, cloud_xyz, want_zbuffer=False)[0]
        flat = self.ctx.fuse_posteriors(index_images, posteriors, cc, n_pts)
        offs = np.cumsum([0] + [c * n_pts for c in cc])
        unaries = [flat[offs[l]:offs[l + 1]].reshape(n_pts, cc[l]) for l in range(len(cc))]
        unknown = unknown_labels if unknown_labels is not None else [p.unknown_label[l] for l in range(len(cc))]
        labels = []
        if p.use_dense_crf:
            pairwise = np.concatenate([cloud_xyz * np.float32(p.dcrf_xyz_kernel), cloud_rgb * np.float32(p.dcrf_rgb_kernel)], 1)   # :629-637
            for l in range(len(cc)):
                _, mp = self.ctx.crf_infer(-unaries[l], pairwise, p.dcrf_kernel_weight, p.dcrf_iterations, capi.LABEL_CRF, unknown[l])
                labels.append(mp.astype(np.uint8))
        else:
            for l in range(len(cc)):
                labels.append(self.ctx.label_values(unaries[l], capi.LABEL_NOCRF, unknown[l]).astype(np.uint8))
        if local_map_id is not None:
            self.store.store(local_map_id, labels)
        return labels, unaries

    # ---- services (ROS request / response fields as plain values) -----------------------------------
    def srvStoredSemanticsIds(self):
        return self.store.srvStoredSemanticsIds()

    def srvGetLocalMapSegmentation(self, local_map_id, segmentation_layers):
        return self.store.srvGetLocalMapSegmentation(local_map_id, segmentation_layers)

    def srvSegmentationInformation(self):  # :776-791
        return {"layer_names": [l["name"] for l in self.layers],
                "class_counts": [len(l["classes"]) for l in self.layers],
                "class_names": [c[0] for l in self.layers for c in l["classes"]],
                "class_colors": [int(v) for l in self.layers for c in l["classes"] for v in c[1]]}

    def close(self):
        self.ctx.close()


class RgbLabelConversion:
    """RgbLabelConversion (include/rgb_label_conversion.h) for one layer of a context: `coding` is one config.json
    color_codings[*].coding list ({name, color: [r, g, b], label}).  Images convert on the GPU; images are RGB byte
    order (the PNG's), the reference's BGR swaps cancel out.  missing_label: label of colours not in the table -- 0 as
    the reference's std::map gives (rgb_label_conversion.h:86-88), -1 to leave them unscored."""

    def __init__(self, ctx, coding, layer=0, missing_label=0):
        self.ctx, self.layer, self.coding = ctx, layer, list(coding)
        self._name_to_label, self._label_to_name = {}, {}
        for e in self.coding:                      # std::map assignments in entry order (:29-38)
            lab = int(np.int64(e["label"]).astype(np.int8))
            self._name_to_label[e["name"]] = lab
            self._label_to_name[lab] = e["name"]
        ctx.color_coding_set(layer, self.coding, missing_label)

    def rgbToLabel(self, image):                   # :59-78; (H, W, 3) or (n, H, W, 3)
        im = np.asarray(image, np.uint8)
        one = im.ndim == 3
        out = self.ctx.labels_from_rgb(im[None] if one else im, self.layer)
        return out[0] if one else out

    def labelToRgb(self, labels):                  # :42-57; (H, W) or (n, H, W)
        lab = np.asarray(labels, np.int8)
        one = lab.ndim == 2
        out = self.ctx.labels_to_rgb(lab[None] if one else lab, self.layer)
        return out[0] if one else out

    def getLabelName(self, label):                 # :91-93 ("" for an unknown label, as operator[] gives)
        return self._label_to_name.get(int(label), "")

    def getLabelNumber(self, name):                # :95-97 (0 for an unknown name)
        return self._name_to_label.get(name, 0)

    def getValidLabelCount(self):                  # :103-110
        return sum(1 for l in self._label_to_name if l >= 0)


class Evaluator:
    """The scoring of src/test.cpp:182-228 / src/test_multi.cpp:222-268 on the GPU for every label layer of a context:
    `codings` holds one config.json coding list per layer (or None for a layer scored from int8 ground truth only).
    add(pred, gt) takes host arrays, add_device(...) device addresses; counts are uint64 and exact."""

    def __init__(self, ctx, codings, missing_label=0):
        self.ctx = ctx
        self.class_counts = ctx.forest_info()["class_counts"]
        if len(codings) != len(self.class_counts):
            raise ValueError("one coding per label layer of the model (%d)" % len(self.class_counts))
        self.conv = [RgbLabelConversion(ctx, c, l, missing_label) if c is not None else None for l, c in enumerate(codings)]
        ctx.eval_reset()

    def reset(self):
        self.ctx.eval_reset()

    def add(self, pred, gt, gt_format=None):
        self.ctx.eval_accumulate(pred, gt, gt_format)

    def add_device(self, n, d_pred, d_gt, gt_format=capi.GT_LABELS, stream=0):
        self.ctx.eval_accumulate_device(n, d_pred, d_gt, gt_format, stream)

    def confusion(self, layer):
        return self.ctx.eval_confusion(layer)[0]

    def out_of_range(self, layer):
        return self.ctx.eval_confusion(layer)[1]

    def scores(self, layer):
        """dict(global_acc, class_avg_acc, iou, row_pct, counts) as test.cpp:203-228 computes them."""
        counts = self.confusion(layer)
        d = capi.eval_scores_from_counts(counts)
        d["counts"] = counts
        return d

    def report(self, layer):
        """The text test.cpp:206-228 prints (its spelling included)."""
        s = self.scores(layer)
        counts = s["counts"]
        conv = self.conv[layer]
        lines = ["confusion:"]
        for i in range(counts.shape[0]):
            name = conv.getLabelName(i) if conv is not None else ""
            row = name.ljust(15) + "".join(" %6.2f" % v for v in s["row_pct"][i])
            lines.append(row + "   out of %d pixels" % int(counts[i].sum()))
        lines.append("Global accuracy:         %6.2f " % s["global_acc"])
        lines.append("Class averge accuracy:   %6.2f " % s["class_avg_acc"])
        lines.append("Intersection over union: %6.2f " % s["iou"])
        return "\n".join(lines) + "\n"
