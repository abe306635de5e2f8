"""TEST INFRASTRUCTURE ONLY -- a Python restatement of libforest's forest pruning: the simulated-annealing driver
(third-party/libforest/src/mcmc.h:147-240, GeometricCoolingSchedule :272-346) and RandomForestPrune with its moves and
its two energies (todos.txt:51-166, 186-226, 245-297), written from those lines and from the build-owned definitions of
include/rvseg.h ("forest pruning"), independently of the HIP code and of csrc/prune_host.h.

The chain is np.float32 arithmetic step by step; logf comes from libm through ctypes, as in boost_restate.  A run takes
the votes of every tree (T, P) -- or the T x T agree counts for the cover energy -- and returns the whole trajectory."""
import ctypes as C

import numpy as np

import boost_restate as br

F32 = np.float32
EXCHANGE, REMOVE, ADD = 0, 1, 2
ERROR, COVER = 0, 1
MAX_STATE = 64
DEFAULTS = dict(start_temperature=100.0, end_temperature=1e-5, alpha=0.95, inner_loops=250, p_exchange=1.0, p_remove=0.0, p_add=0.0,
                energy=ERROR, seed=0)


# ---- the draws (build-owned): slot k of step s -------------------------------------------------------------------------
def prune_key(seed):
    return br.mix64(seed ^ br.mix64(0x7072756E))


def draw(key, step, slot):
    return br.draw64(key, 4 * step + slot)


def uniform(d):
    """24 random bits, exact in fp32, in [0, 1)."""
    return F32(F32(d >> 40) * F32(2.0 ** -24))


def logf(u):
    return F32(br._libm.logf(C.c_float(float(u))))


# ---- the schedule (mcmc.h:159, 170-173, 312-315) ---------------------------------------------------------------------
def temperatures(start, end, alpha, limit=1 << 22):
    """The temperature of iteration 1, 2, ...: while (temperature > end) { iteration++; temperature *= alpha; ... }."""
    out = []
    t, end, alpha = F32(start), F32(end), F32(alpha)
    while t > end:
        t = F32(t * alpha)
        out.append(t)
        assert len(out) <= limit
    return out


# ---- the moves -----------------------------------------------------------------------------------------------------------
def registered_moves(p):
    """addMove in the order exchange, remove, add; a move of probability 0 is not registered."""
    return [(kind, F32(p[name])) for kind, name in ((EXCHANGE, "p_exchange"), (REMOVE, "p_remove"), (ADD, "p_add")) if p[name] > 0]


def choose_move(moves, u):
    """mcmc.h:178-198."""
    prob_sum = F32(0)
    for kind, prob in moves:
        if prob_sum <= u and u < F32(prob_sum + prob):
            return kind
        prob_sum = F32(prob_sum + prob)
    return moves[-1][0]


def propose(kind, state, d_tree, d_pos, T):
    """todos.txt:58-87 (remove), :110-118 (add; a state of MAX_STATE entries is copied: build-owned), :141-155 (exchange)."""
    new = list(state)
    if kind == EXCHANGE:
        new[d_pos % len(state)] = d_tree % T
    elif kind == REMOVE:
        if len(state) >= 2:
            del new[d_pos % len(state)]
    elif len(state) < MAX_STATE:
        new.append(d_tree % T)
    return new


# ---- the energies --------------------------------------------------------------------------------------------------------
def predictions(votes, state, n_classes=256, rule="first"):
    """todos.txt:193-214 per point: the label whose count first exceeds the running maximum (0 with 0 votes to start).
    rule="lowest": the lowest label among the most voted, which the reference does NOT compute (for the tie case)."""
    votes = np.asarray(votes)
    P = votes.shape[1]
    rows = np.arange(P)
    count = np.zeros((P, n_classes), np.int64)
    max_votes = np.zeros(P, np.int64)
    max_label = np.zeros(P, np.int64)
    for t in state:
        v = votes[t].astype(np.int64)
        count[rows, v] += 1
        win = count[rows, v] > max_votes
        max_votes[win] = count[rows, v][win]
        max_label[win] = v[win]
    if rule == "lowest":
        return np.where(max_votes > 0, count.argmax(1), 0)
    return max_label


def error_count(votes, labels, state, rule="first"):
    return int((predictions(votes, state, rule=rule) != np.asarray(labels, np.int64)).sum())


def error_energy(votes, labels, state):
    """todos.txt:216-225: a float grown by += 1 (it stops at 2^24) over the number of points."""
    return F32(F32(min(error_count(votes, labels, state), 1 << 24)) / F32(np.asarray(votes).shape[1]))


def cover_energy(agree, P, state):
    """todos.txt:281-297 on distances[i][j] = P - agree[i][j]."""
    dist = np.int64(P) - np.asarray(agree, np.uint64).astype(np.int64)
    res = int(dist[list(state)].min(0).sum())
    return F32(F32(res) / F32(len(state)))


# ---- the chain (mcmc.h:147-240) ----------------------------------------------------------------------------------------
def run(params, T, state, energy):
    """params: the fields of rvseg_prune_params over DEFAULTS; energy(state) -> np.float32.  Returns dict(state = the best
    state, best_energy, trace = [(iteration, temperature, energy, best_energy, state_size)], step_kind, and for the recipes'
    own claims: improvement per step, moves = (kind, len(state) before) per step, final = the last current state)."""
    p = dict(DEFAULTS, **params)
    key = prune_key(p["seed"])
    moves = registered_moves(p)
    state = [int(t) for t in state]
    current = energy(state)
    best, best_state = current, list(state)
    trace, kinds, improvements, drawn = [], [], [], []
    s = 0
    for iteration, temperature in enumerate(temperatures(p["start_temperature"], p["end_temperature"], p["alpha"]), 1):
        for _ in range(p["inner_loops"]):
            kind = choose_move(moves, uniform(draw(key, s, 0)))
            drawn.append((kind, len(state)))
            new = propose(kind, state, draw(key, s, 1), draw(key, s, 2), T)
            new_energy = energy(new)
            improvement = F32(new_energy - current)
            improvements.append(improvement)
            if improvement <= 0:
                accepted = 1
            else:
                with np.errstate(divide="ignore"):
                    accepted = 2 if logf(uniform(draw(key, s, 3))) <= F32(F32(-improvement) / temperature) else 0
            if accepted:
                current, state = new_energy, new
            if current < best:
                best, best_state = current, list(state)
            kinds.append(accepted)
            s += 1
        trace.append((iteration, temperature, current, best, len(state)))
    return dict(state=np.asarray(best_state, np.int32), best_energy=F32(best), trace=trace, step_kind=np.asarray(kinds, np.uint8),
                improvement=np.asarray(improvements, F32), moves=drawn, final=np.asarray(state, np.int32))


def trace_array(trace):
    out = np.zeros(len(trace), np.dtype([("iteration", np.int32), ("temperature", F32), ("energy", F32), ("best_energy", F32),
                                         ("state_size", np.int32)]))
    for i, row in enumerate(trace):
        out[i] = row
    return out
