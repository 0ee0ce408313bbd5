"""Inputs, references, mutants and the tables of cases of tests/test_gpu_moe_exact.py: the exact-sum contract of tests/exact_cases.py
(fp32 accumulation, ONE rounding, nothing lost, doubled or shifted -- held bit for bit) on the routed mixture-of-experts kernels:
the grouped decode kernel (moe_gemm_kernel.hpp behind eetq_w8a16_moe_gemm / eetq_w4a16_moe_gemm), the grouped tiled prompt kernels,
the grouped input-gradient kernels and the weighted combine.  NumPy only, no GPU.

One expert is one exact_cases.Problem: Weight(case, index = e) gives every expert its own codes and its own scales, the activations
are those of exact_cases, and the level of the ladder is chosen from the shape as there.  A Routed problem lays the experts' rows out
in the sorted order of the routing tables; rows at or past offsets[E] hold POISON (what the output buffer was filled with).

The decode kernel's K loop is its own (wave w owns k tiles w, w + WAVES, ...; D stages in flight; a tail of r = n - (i + D) clamped
loads consumed under `if (d < r)`; an fp32 cross-wave reduction through LDS per 16 rows of an expert), so every K of DECODE_K is
listed with the (waves, depth) it selects and the tiles every wave owns.  plan() RESTATES the two plan rules (moe.hip, moe_int4.hip,
no tuning variable set): the library has no host query for the MoE plan, so what rests on plan() is unverified against the library
(a rule that changed there would leave these K values exact but possibly off the seams they are listed for).

Combine inputs: y[p][h] = i / 64 with |i| <= 2047, weights m / 16 with m in 0 .. 16: both exact in fp16, every product an integer
number of quanta 2^-10, a token's sum of magnitudes at most 8 * 2047 * 16 < 2^18 quanta -- the fp32 accumulator is exact whether or not
the compiler fuses the multiply and the add, and the result must equal fp16(exact sum)."""
from collections import namedtuple

import numpy as np

import exact_cases as ec
from exact_cases import LADDER, LIMIT, MUTANT_FLOOR, Problem, Weight, activations, as_x, level, mutants  # noqa: F401  (reused as they are)

E, TOPK, N = 8, 2, 48        # N = 48: a first, a middle and a last 16-column tile row, and 24 gated columns
COUNTS = (0, 1, 15, 16, 17, 33, 0, 2)
POISON = -777.0


# ---------------------------------------------------------------------------------------------------------------- routing
class Route:
    """The tables eetq_moe_route builds from idx [T, k] (a stable sort of the slots by expert; ids outside 0 .. E - 1 get no row)"""

    def __init__(self, idx, experts=E):
        self.idx, self.E = np.asarray(idx, np.int64), experts
        self.T, self.k = self.idx.shape
        flat = self.idx.ravel()
        self.S = flat.size
        valid = (flat >= 0) & (flat < experts)
        self.counts = np.bincount(flat[valid], minlength=experts).astype(np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        order = np.argsort(np.where(valid, flat, experts), kind="stable")
        self.used = int(valid.sum())
        self.sorted_slot = np.full(self.S, -1, np.int32)
        self.sorted_slot[:self.used] = order[:self.used]
        self.position = np.full(self.S, -1, np.int32)
        self.position[order[:self.used]] = np.arange(self.used, dtype=np.int32)
        act = np.flatnonzero(self.counts)
        self.active = np.full(min(experts, self.S), -1, np.int32)
        self.active[:act.size] = act

    def live(self):
        return [e for e in range(self.E) if self.counts[e]]

    def span(self, e):
        return slice(int(self.offsets[e]), int(self.offsets[e + 1]))

    def slots(self, e):
        return self.sorted_slot[self.span(e)].astype(np.int64)

    def tokens(self, e):
        return self.slots(e) // self.k

    def expert_of_row(self):
        out = np.full(self.S, -1)
        for e in self.live():
            out[self.span(e)] = e
        return out


def decode_routing():
    """E = 8, k = 2, counts COUNTS, one slot with id E and one with -1 (offsets[E] = 84 < S = 86), shuffled from a fixed seed"""
    flat = np.concatenate([np.full(c, e) for e, c in enumerate(COUNTS)] + [[E], [-1]]).astype(np.int64)
    flat = flat[np.random.default_rng(20240601).permutation(flat.size)]
    return Route(flat.reshape(-1, TOPK))


def straddle_routing(idx):
    """tests/test_gpu_moe_prompt.py's `straddle` ids (T = 385, k = 1, counts 127, 128, 129, 1), as that test draws them"""
    r = Route(np.asarray(idx), E)
    assert (r.T, r.k) == (385, 1) and sorted(r.counts.tolist()) == [0, 0, 0, 0, 1, 127, 128, 129]
    return r


# ---------------------------------------------------------------------------------------------------------------- the plan
def plan(bits, K):
    """(waves, stages in flight) of eetq_w8a16_moe_gemm (moe.hip) / eetq_w4a16_moe_gemm (moe_int4.hip), restated"""
    kt = K // tile_k(bits)
    if bits == 8:
        return (8, 2) if kt >= 16 else (4, 2) if kt >= 8 else (1, 1)
    return (8, 2) if kt >= 64 else (4, 1) if kt >= 4 else (2, 1) if kt >= 2 else (1, 1)


def tile_k(bits):
    return 64 if bits == 8 else 128


def tiles_per_wave(bits, K):
    waves, _ = plan(bits, K)
    kt = K // tile_k(bits)
    return tuple((kt - w + waves - 1) // waves for w in range(waves))


def loop_shape(n, depth):
    """the kernel's K loop on a wave that owns n tiles: (iterations of the steady loop, r = tail stages consumed)"""
    i = steady = 0
    while i + 2 * depth <= n:
        i, steady = i + depth, steady + 1
    return steady, n - (i + depth)


def features(bits, K):
    """what a K exercises of its instantiation: tail stages consumed, unequal tile counts, the steady loop running or not"""
    waves, depth = plan(bits, K)
    ns = tiles_per_wave(bits, K)
    assert min(ns) >= depth, "a wave with fewer tiles than stages in flight"
    out = set()
    for n in ns:
        steady, r = loop_shape(n, depth)
        assert 0 <= r <= depth - 1                 # the tail holds D - 1 stages
        out.add(("steady", steady > 0))
        if depth > 1:
            out.add(("r", r))
    if len(set(ns)) > 1:
        out.add(("unequal",))
    return out


def reachable(bits, waves, depth, k_max=16384):
    """every feature some K <= k_max shows on the instantiation (a form with one K, or none below 4 tiles per wave, cannot show all)"""
    out = set()
    for K in range(tile_k(bits), k_max + 1, tile_k(bits)):
        if plan(bits, K) == (waves, depth):
            out |= features(bits, K)
    return out


DECODE_K = {8: (64, 448, 512, 576, 960, 1024, 1088, 1984, 2112), 4: (128, 256, 384, 512, 640, 896, 8064, 8192, 8320, 9088)}
# what the issue lists each K for: (waves, depth), tiles per wave (first wave, last wave)
LISTED = {(8, 64): ((1, 1), (1, 1)), (8, 448): ((1, 1), (7, 7)), (8, 512): ((4, 2), (2, 2)), (8, 576): ((4, 2), (3, 2)), (8, 960): ((4, 2), (4, 3)),
          (8, 1024): ((8, 2), (2, 2)), (8, 1088): ((8, 2), (3, 2)), (8, 1984): ((8, 2), (4, 3)), (8, 2112): ((8, 2), (5, 4)),
          (4, 128): ((1, 1), (1, 1)), (4, 256): ((2, 1), (1, 1)), (4, 384): ((2, 1), (2, 1)), (4, 512): ((4, 1), (1, 1)), (4, 640): ((4, 1), (2, 1)),
          (4, 896): ((4, 1), (2, 1)), (4, 8064): ((4, 1), (16, 15)), (4, 8192): ((8, 2), (8, 8)), (4, 8320): ((8, 2), (9, 8)), (4, 9088): ((8, 2), (9, 8))}

DecodeCase = namedtuple("DecodeCase", "id bits K waves depth tiles case")


def _decode_case(bits, K, T):
    waves, depth = plan(bits, K)
    tiles = tiles_per_wave(bits, K)
    form = "moe_gemm_kernel<%d, %d, %d>, k tiles per wave %s" % (bits, waves, depth, "/".join(map(str, tiles)))
    case = ec._case("moe-decode-i%d-k%d" % (bits, K), "moe", T, K, N, None, form, ("none", None), bits=bits)
    return DecodeCase(case.id, bits, K, waves, depth, tiles, case)


DECODE_T = decode_routing().T
DECODE_CASES = [_decode_case(bits, K, DECODE_T) for bits in (8, 4) for K in DECODE_K[bits]]

# tiled prompt kernels: the ring minimum (int8 K = 320 = kMinKSteps steps of 64; int4 K = 384) and the step counts just above it
TILED_N = 272
TILED_K = {8: (320, 384, 448), 4: (384, 512, 640)}
TILED_CASES = [ec._case("moe-tiled-i%d-k%d" % (bits, K), "moe", 385, K, TILED_N, None, "grouped tiled prompt kernel, %d K steps of 64" % (K // 64),
                        ("none", None), bits=bits) for bits in (8, 4) for K in TILED_K[bits]]
# grouped input gradient: both tails (K % 128 == 64, N % 64 == 16; the int4 layout needs K % 128 == 0), rows in sorted order
GRAD_CASES = [ec._case("moe-grad-i%d-%dx272" % (bits, K), "moe", DECODE_T * TOPK, K, 272, None, "grouped w%d_a16 input gradient" % bits, ("none", None),
                       bits=bits, op="gemm_t") for bits, K in ((8, 320), (4, 384))]


# ---------------------------------------------------------------------------------------------------------------- routed problems
class Routed:
    """Every live expert's Problem under a Route.  Forward: x [T, K] (exact_cases.activations), expert e's rows are its tokens in
    sorted order.  Gradient (case.op == "gemm_t"): dy [S, N] already in sorted order, expert e's rows are its span."""

    def __init__(self, case, route):
        self.case, self.route = case, route
        self.i = activations(case)
        assert self.i.shape[0] == (route.S if case.op == "gemm_t" else route.T)
        self.w = [Weight(case, e) for e in range(route.E)]
        self.p = {e: Problem(case, self.w[e], self.i, self.rows(e)) for e in route.live()}
        self.cols = case.K if case.op == "gemm_t" else case.N

    def rows(self, e):
        return np.arange(*self.route.span(e).indices(self.route.S)) if self.case.op == "gemm_t" else self.route.tokens(e)

    def assemble(self, fn):
        """[S, cols] fp16: fn(e, Problem) on every live expert's rows, POISON at and past offsets[E]"""
        y = np.full((self.route.S, self.cols), POISON, np.float16)
        for e, p in self.p.items():
            y[self.route.span(e)] = fn(e, p)
        return y

    def reference(self):
        return self.assemble(lambda e, p: p.reference())

    def bound(self):
        return max(float(p.bound().max()) for p in self.p.values())

    def quantum(self):
        q = np.ones((self.route.S, self.cols))
        for e, p in self.p.items():
            q[self.route.span(e)] = p.quantum[None, :]
        return q

    def sorted_x(self):
        """the gather = 0 input: the tokens' rows in sorted order, NaN at and past offsets[E]"""
        x = np.full((self.route.S, self.case.K), np.nan, np.float16)
        x[:self.route.used] = as_x(self.i)[self.route.sorted_slot[:self.route.used] // self.route.k]
        return x


def decode_mutants(rp, dc):
    """{name: ([S, N] fp16 of a kernel that breaks the contract in one way, the rows the fault touches)}.  exact_cases.mutants runs
    on the rows of the 33-row expert (three 16-row groups); the others are the decode kernel's and the routing's own faults."""
    r, case, tile = rp.route, rp.case, tile_k(dc.bits)
    ref = rp.reference()
    live_rows = np.arange(r.used)
    out = {}
    big = int(np.argmax(r.counts))
    for name, y in mutants(rp.p[big]).items():
        full = ref.copy()
        full[r.span(big)] = y
        out[name] = (full, np.arange(*r.span(big).indices(r.S)))
    # ONE product is quietest where one row decides what quiet is: the 1-row expert (over 33 rows every k has a large |x| somewhere)
    one = int(np.flatnonzero(r.counts == 1)[0])
    for name, y in mutants(rp.p[one]).items():
        if name in ("lost_quietest_k", "doubled_quietest_k"):
            full = ref.copy()
            full[r.span(one)] = y
            out[name + "_of_the_1_row_expert"] = (full, np.arange(*r.span(one).indices(r.S)))
    last = (dc.waves - 1) + (dc.tiles[-1] - 1) * dc.waves       # the last k tile of the last wave
    tail0 = (dc.tiles[0] - 1) * dc.waves                        # wave 0's last tile: its tail stage where r = 1

    def tile_sum(p, t):
        return p.sums(None, t * tile, (t + 1) * tile)

    out["last_tile_of_last_wave_lost"] = (rp.assemble(lambda e, p: p.f16(p.sums() - tile_sum(p, last))), live_rows)
    out["last_tile_of_last_wave_doubled"] = (rp.assemble(lambda e, p: p.f16(p.sums() + tile_sum(p, last))), live_rows)
    out["tail_tile_of_wave_0_lost"] = (rp.assemble(lambda e, p: p.f16(p.sums() - tile_sum(p, tail0))), live_rows)
    if dc.waves > 1:
        def wave_partials(e, p):
            acc = np.zeros((p.a.shape[0], case.N), np.float32)
            for w in range(dc.waves):                           # fp16(partial) of every wave, added in fp32 in wave order
                a = np.zeros_like(p.a)
                for t in range(w, case.K // tile, dc.waves):
                    a[:, t * tile:(t + 1) * tile] = p.a[:, t * tile:(t + 1) * tile]
                acc = acc + p.f16(p.sums(a)).astype(np.float32)
            return acc.astype(np.float16)
        out["fp16_wave_partials"] = (rp.assemble(wave_partials), live_rows)
    out["weight_of_next_expert"] = (rp.assemble(lambda e, p: Problem(case, rp.w[(e + 1) % r.E], rp.i, rp.rows(e)).reference()), live_rows)

    def next_scales(e, p):
        v, nxt = Weight.__new__(Weight), rp.w[(e + 1) % r.E]
        v.q, v.c4, v.e, v.s = rp.w[e].q, nxt.c4, nxt.e, nxt.s
        return Problem(case, v, rp.i, rp.rows(e)).reference()
    out["scales_of_next_expert"] = (rp.assemble(next_scales), live_rows)
    # x[sorted_slot[p]] in place of x[sorted_slot[p] / k] (slots at or past T wrap: the kernel would read past x)
    out["x_row_of_the_slot"] = (rp.assemble(lambda e, p: Problem(case, rp.w[e], rp.i, r.slots(e) % r.T).reference()), live_rows)
    full, touched = ref.copy(), []
    for e in r.live():                                          # the clamped row `rows - 1` of a ragged 16-row group stored to row `rows`
        if r.counts[e] % 16:
            full[r.offsets[e + 1]] = ref[r.offsets[e + 1] - 1]
            touched.append(int(r.offsets[e + 1]))
    out["clamped_row_stored_one_past"] = (full, np.array(touched))
    return out


def tier_a_accepts(rp, y, ref):
    """what the tier-A tests do with the result: every live expert's rows against the reference, and the rows past offsets[E] untouched"""
    from act_cases import tier_a
    r = rp.route
    return all(tier_a(y[r.span(e)], ref[r.span(e)]).all() for e in r.live()) and np.array_equal(y[r.used:], ref[r.used:])


# ---------------------------------------------------------------------------------------------------------------- combine
CombineCase = namedtuple("CombineCase", "id T k H wdtype")
COMBINE_CASES = [CombineCase("combine-t%d-k%d-h%d-%s" % (T, k, H, wd), T, k, H, wd)
                 for T in (1, 5) for k in (1, 2, 8) for H in (8, 2040, 2048, 2056) for wd in ("f32", "f16")]
Y_SHIFT, W_SHIFT = 6, 4      # y = i / 2^6, w = m / 2^4: a product is i m quanta of 2^-10
SPARE = 3                    # rows of y that no position names: NaN


class Combine:
    """i: int64 [P, H] (|i| <= 2047), m: int64 [T, k] (0 .. 16), position: int32 [T k] with -1 among them.  T = 5: token 2 has no live
    slot (its output is zeros) and, from k = 2 on, token 0 has lost its FIRST slot (a `break` in place of the `continue` drops the
    rest).  m is uniform in 0 .. 16, except that a token's only live slot weighs at least 1 / 16 (dropping it shows) and the first two
    live slots of a token take an m that is no power of two (their products need more than fp16's 11 bits: an early rounding shows)."""

    def __init__(self, c):
        # At H = 8 a token is eight elements, and whether an early rounding shows on one of them is a matter of the draw: the first draw
        # on which every mutant shows on >= MUTANT_FLOOR of the elements it touches is taken (a property of the inputs and the
        # reference models alone; tests/test_moe_exact_cases_cpu.py asserts it of the draw that is used).
        for attempt in range(32):
            self._draw(c, attempt)
            want = self.reference()
            if all(ec.differs(y[self.touched(name)], want[self.touched(name)]) >= MUTANT_FLOOR for name, y in self.mutants().items()):
                return
        raise AssertionError("no draw of %s shows every mutant" % c.id)

    def _draw(self, c, attempt):
        self.c = c
        rng = np.random.default_rng([c.T, c.k, c.H, 11, attempt])
        S = c.T * c.k
        P = S + SPARE
        self.i = rng.integers(-2047, 2048, size=(P, c.H))
        self.m = rng.integers(0, 17, size=(c.T, c.k))
        pos = rng.permutation(P)[:S].astype(np.int32).reshape(c.T, c.k)
        if c.T > 1:
            pos[2, :] = -1
            if c.k > 1:
                pos[0, 0] = -1
        self.live = pos >= 0
        for t in range(c.T):
            lv = np.flatnonzero(self.live[t])
            if len(lv) >= 2:         # i m is an fp16 value whenever m is 0 or a power of two: an early rounding rounds nothing then
                self.m[t, lv[:2]] = rng.choice(np.array([3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15]), 2, replace=False)    # two different ones
            elif len(lv) == 1 and self.m[t, lv[0]] == 0:
                self.m[t, lv[0]] = 16
        self.position = pos.ravel()
        named = np.zeros(P, bool)
        named[self.position[self.position >= 0]] = True
        self.y = (self.i / 2.0 ** Y_SHIFT).astype(np.float16)
        assert np.array_equal(self.y.astype(np.float64) * 2 ** Y_SHIFT, self.i)
        self.y[~named] = np.nan
        self.w = (self.m / 2.0 ** W_SHIFT).astype(np.float32 if c.wdtype == "f32" else np.float16)
        assert np.array_equal(self.w.astype(np.float64) * 2 ** W_SHIFT, self.m)
        self.quantum = 2.0 ** -(Y_SHIFT + W_SHIFT)

    def products(self, m=None):
        """[T, k, H] in quanta; 0 for a slot with position -1"""
        m = self.m if m is None else m
        pos = self.position.reshape(self.c.T, self.c.k)
        return np.where(self.live[:, :, None], self.i[np.maximum(pos, 0)] * m[:, :, None], 0)

    def bound(self):
        return int(np.abs(self.products()).sum(1).max())

    def f16(self, quanta):
        return (quanta * self.quantum).astype(np.float16)

    def reference(self):
        return self.f16(self.products().sum(1).astype(np.float64))

    def touched(self, name):
        """tokens on which the mutant can show: a live slot to drop; two live slots for an early rounding or a neighbour's weight"""
        n = self.live.sum(1)
        return np.flatnonzero(n >= (1 if name == "dropped_slot" else 2))

    def mutants(self):
        c, pr = self.c, self.products()
        heavy = np.argmax(self.m * self.live, axis=1)
        keep = np.ones((c.T, c.k), bool)
        keep[np.arange(c.T), heavy] = False
        out = {"dropped_slot": self.f16((pr * keep[:, :, None]).sum(1).astype(np.float64))}
        if c.k > 1:
            out["weight_of_next_slot"] = self.f16(self.products(np.roll(self.m, -1, axis=1)).sum(1).astype(np.float64))
            early = np.zeros((c.T, c.H), np.float32)
            acc16 = np.zeros((c.T, c.H), np.float16)
            for j in range(c.k):
                early = early + self.f16(pr[:, j].astype(np.float64)).astype(np.float32)
                acc16 = (acc16.astype(np.float32) + (pr[:, j] * self.quantum).astype(np.float32)).astype(np.float16)
            out["products_rounded_to_fp16"] = early.astype(np.float16)
            out["fp16_accumulator"] = acc16
        return out
