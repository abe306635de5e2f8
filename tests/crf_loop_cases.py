"""What the learning-loop tests share: the synthetic scene of the dense_learning recipe, and the evaluation path that existed
before rvseg_crf_model_energy_gradient (a fresh model for every evaluation, composed call by call) as the reference."""
import numpy as np

f32 = np.float32
W, H, M, NIT = 48, 32, 4, 5
PHASES = [(True, False, False), (True, True, False), (True, True, True)]


def scene():
    rng = np.random.default_rng(5)
    gt = np.full((H, W), -1, np.int16)   # three labelled blocks, the rest unlabelled
    gt[2:14, 3:20] = 0
    gt[4:28, 26:44] = 1
    gt[18:30, 2:22] = 2
    colours = np.array([[200, 40, 40], [40, 190, 60], [50, 60, 210], [128, 128, 128]], np.float64)
    im = colours[np.where(gt < 0, 3, gt)] + rng.normal(0, 25, (H, W, 3))
    im = np.clip(im, 0, 255).astype(np.uint8)
    f = np.ones((W * H, 4), f32)
    f[:, :3] = (im.reshape(-1, 3) / 255.).astype(f32)   # logistic features [r, g, b, 1]
    L = (0.01 * (1 - 2 * rng.random((M, 4)))).astype(f32)
    return im, gt.reshape(-1), f, L


class ParentEnergy:
    """CRFKernelEnergy over ParentPath (tests/test_gpu_crf_model_params.py)."""

    def __init__(self, parent, flags, l2):
        self.parent, self.flags, self.l2 = parent, flags, l2
        nu, nc, nk = parent.counts()
        rv = parent.rv
        kp = [np.zeros(0, f32) if t[2] == rv.CONST_KERNEL else t[4] if t[4] is not None else
              np.ones(t[0].shape[1], f32) if t[2] == rv.DIAG_KERNEL else np.eye(t[0].shape[1], dtype=f32).reshape(-1) for t in parent.terms]
        groups = [np.ascontiguousarray(parent.L.T).reshape(-1), np.concatenate([t[1].parameters() for t in parent.terms]), np.concatenate(kp)]
        self.x0 = np.concatenate([g for on, g in zip(flags, groups) if on]).astype(f32)

    def initialValue(self):
        return self.x0

    def gradient(self, x):
        return self.parent.gradient(x, *self.flags, self.l2)


class ParentPath:
    """CRFKernelEnergy.gradient as it was before the one entry: every evaluation uploads the logistic unary it has read back and
    sets the model afresh, then composes gradient(_kernel) and logistic_gradient in Python."""

    def __init__(self, rv, ctx, L, f, terms, obj, nit):
        self.rv, self.ctx, self.L, self.f, self.obj, self.nit = rv, ctx, L.copy(), f, obj, nit
        self.terms = [list(t) for t in terms]
        self.evaluations = 0

    def counts(self):
        rv = self.rv
        return (self.L.size, [t[1].parameters().shape[0] for t in self.terms],
                [0 if t[2] == rv.CONST_KERNEL else t[0].shape[1] if t[2] == rv.DIAG_KERNEL else t[0].shape[1] ** 2 for t in self.terms])

    def set(self, x, unary, pairwise, kernel):
        nu, nc, nk = self.counts()
        i = 0
        if unary:
            self.L = np.ascontiguousarray(x[:nu].reshape(self.L.shape[1], self.L.shape[0]).T)
            i = nu
        if pairwise:
            for t, n in zip(self.terms, nc):
                t[1].setParameters(x[i:i + n])
                i += n
        if kernel:
            for t, n in zip(self.terms, nk):
                if n:
                    t[4] = x[i:i + n].copy()
                i += n
        assert i == x.shape[0]

    def gradient(self, x, unary, pairwise, kernel, l2):
        x = np.asarray(x, f32)
        self.set(x, unary, pairwise, kernel)
        ctx = self.ctx
        self.evaluations += 1
        ctx.crf_model_set(ctx.crf_logistic_unary(self.L, self.f), [tuple(t) for t in self.terms])
        if kernel:
            r, ug, cg, kg, _ = ctx.crf_model_gradient_kernel(self.nit, self.obj, unary, pairwise)
        else:
            r, ug, cg, _ = ctx.crf_model_gradient(self.nit, self.obj, unary, pairwise)
            kg = None
        parts = []
        if unary:
            parts.append(-ctx.crf_logistic_gradient(ug, self.f).astype(f32))
        if pairwise:
            parts.append(-cg.astype(f32))
        if kernel:
            parts.append(-kg.astype(f32))
        dx = np.concatenate(parts).astype(f32)
        r = -r
        l2 = f32(l2)
        if l2 > 0:
            dx = (dx + l2 * x).astype(f32)
            s = 0.0
            for v in x:   # ascending, in double
                s += float(v) * float(v)
            r += (0.5 * float(l2)) * s
        return r, dx


def reference_loop(rv, ctx, obj, im, f, L, restart=2, max_iterations=8, l2=1e-3):
    """The three phases over ParentPath on `ctx`: the learned (unary, label compatibility, kernel) parameters, float32."""
    gauss = rv.capi.crf_features_gaussian(W, H, 3, 3)
    bil = rv.capi.crf_features_bilateral(W, H, 80, 80, 13, 13, 13, im)
    parent = ParentPath(rv, ctx, L, f, [(gauss, rv.PottsCompatibility(1), rv.DIAG_KERNEL, rv.NORMALIZE_SYMMETRIC, None),
                                        (bil, rv.MatrixCompatibility(np.eye(M, dtype=f32)), rv.DIAG_KERNEL, rv.NORMALIZE_SYMMETRIC, None)], obj, NIT)
    for flags in PHASES:
        parent.set(rv.minimizeLBFGS(ParentEnergy(parent, flags, l2), restart, max_iterations=max_iterations), *flags)
    return ParentEnergy(parent, (True, True, True), l2).initialValue()
