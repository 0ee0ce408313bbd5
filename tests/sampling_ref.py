"""float64 NumPy restatement of the sampling contract of eetq_sample_handover_f16 (include/eetq_amd.h), and a
NumPy Philox4x32-10.  A plain module for the tests (not a conftest)."""
import numpy as np

PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (Python ints) -> 4 output words."""
    c0, c1, c2, c3 = (int(x) & MASK32 for x in counter)
    k0, k1 = (int(x) & MASK32 for x in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK32, p1 & MASK32, ((p0 >> 32) ^ c3 ^ k1) & MASK32, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c0, c1, c2, c3


def philox_uniform(seed, column, row):
    """The kernel's own random number of (seed, column, row): (x0 >> 8) * 2^-24."""
    seed, column = int(seed) & 0xFFFFFFFFFFFFFFFF, int(column) & 0xFFFFFFFFFFFFFFFF
    x0 = philox4x32_10((column & MASK32, column >> 32, row, 0), (seed & MASK32, seed >> 32))[0]
    return np.float32((x0 >> 8) * 2.0 ** -24)


def greedy_token(row):
    """First index of the maximum, NaN counts as the maximum (torch.argmax)."""
    v = np.asarray(row, dtype=np.float64)
    nan = np.isnan(v)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(v))


class Sampled:
    """One row under one setting.  Fields:
    special   : None, "posinf" or "empty" (steps 2 and 3 of the contract: `token` is fixed then)
    classes   : distinct values of the kept entries, descending (float64 logits, not z)
    class_mass: probability of each class (softmax over the top-k survivors, BEFORE top-p renormalisation)
    kept      : boolean mask over the row
    order     : indices of the survivors, by value descending then index ascending
    lo, hi    : cumulative probability interval of each survivor in `order` after renormalisation
    p_margin  : least distance of top_p from a class boundary of the top-k softmax (inf when top-p is off)"""

    def token(self, u):
        if self.special is not None:
            return self.fixed
        hit = np.nonzero(self.hi > float(u))[0]
        return int(self.order[hit[0]] if hit.size else self.order[-1])


def sample_row(row, temperature, top_k=0, top_p=1.0):
    v = np.asarray(row, dtype=np.float64).copy()
    V = v.size
    v[np.isnan(v)] = -np.inf
    r = Sampled()
    r.special, r.p_margin = None, np.inf
    if v.max() == np.inf:
        r.special, r.fixed = "posinf", int(np.argmax(v == np.inf))
        return r
    if v.max() == -np.inf:
        r.special, r.fixed = "empty", 0
        return r
    z = v / np.float64(np.float32(temperature))
    kept = v > -np.inf
    if 0 < top_k < V:
        kept &= v >= np.sort(v)[V - top_k]           # ties at the threshold all stay
    w = np.where(kept, np.exp(z - z.max()), 0.0)
    w /= w.sum()                                     # softmax over the top-k survivors
    classes = np.unique(v[kept])[::-1]               # descending; -0 == +0
    mass = _class_mass(v, w, classes)
    if 0.0 < top_p < 1.0:
        before = np.concatenate([[0.0], np.cumsum(mass)[:-1]])
        stay = before < np.float64(np.float32(top_p))
        if before.size > 1:
            r.p_margin = float(np.abs(before[1:] - np.float64(np.float32(top_p))).min())
        classes, mass = classes[stay], mass[stay]
        kept &= v >= classes[-1]
    r.classes, r.class_mass, r.kept = classes, mass, kept
    idx = np.nonzero(kept)[0]
    order = idx[np.lexsort((idx, -v[idx]))]
    p = w[order] / w[order].sum()
    r.order, r.hi = order, np.cumsum(p)
    r.lo = r.hi - p
    return r


def _class_mass(v, w, classes):
    pos = np.searchsorted(-classes, -v)              # class of every entry (entries outside the kept set carry w = 0)
    pos = np.clip(pos, 0, classes.size - 1)
    return np.bincount(pos, weights=w, minlength=classes.size)
