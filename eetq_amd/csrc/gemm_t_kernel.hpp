// Kernel template of the projection's input gradient dx[M][K] = fp16( sum_n dy[M][n] * fp16(q[k][n] * s[n]) ) (included by
// gemm_t.hip, BITS = 8 plain and grouped, gemm_t_int4.hip, BITS = 4 plain, and moe_gemm_t_int4.hip, BITS = 4 grouped).  The tile, the LDS images, the pipeline and the epilogue are described
// in gemm_t.hip's header; the two BITS differ only in the weight PRODUCER (global load -> dequant -> fp16 image rows), see `store`.
#pragma once
#include "common.hpp"

namespace eetq {
namespace gemm_t {

constexpr int BM = 128, BK = 128, BN = 64;        // dx rows, dx columns (k), reduction step (n)
constexpr int Y_BYTES     = BM * BN * 2;          // 16 KiB: dy stage, 128-byte rows
constexpr int W_BYTES     = BN * BK * 2;          // 16 KiB: fp16 weight image, rows = n, 256-byte rows of k
constexpr int STAGE_BYTES = Y_BYTES + W_BYTES;
constexpr int SMEM_BYTES  = 2 * STAGE_BYTES;      // 64 KiB: no large-LDS opt-in, two workgroups per CU
constexpr int kOutRow     = BK + 8;               // halfs per row of the output image (272 B: bank shift per row)
static_assert(BM * kOutRow * 2 <= SMEM_BYTES, "the output image must fit in the stages");

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
typedef __attribute__((address_space(3))) u32x2 lds_u32x2;
typedef __attribute__((address_space(3))) void  lds_void;

__device__ __forceinline__ lds_u32x4* lds16(int addr) { return (lds_u32x4*)(uintptr_t)(uint32_t)addr; }

// byte offset of 16-byte chunk ch (0..15) of row `row` in the weight image
__device__ __forceinline__ int w_off(int row, int ch) { return row * 256 + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }
// byte offset of 16-byte chunk ch (0..7) of row `row` in the dy stage
__device__ __forceinline__ int y_off(int row, int ch) { return row * 128 + 16 * (ch ^ ((row >> 1) & 7)); }

// The int4 producer's dequantiser: dequant_16_i4's values (gemm_kernel.hpp: k-locals 0..15 of one column from two dwords, nibble
// positions [0, 4, 1, 5, 2, 6, 3, 7], fp16(q) * scale with one rounding) with the unpack done as dequant_dword does it for bytes.
// Per dword, w & 0x0f0f0f0f holds nibbles 0, 2, 4, 6 as bytes and (w >> 4) & 0x0f0f0f0f nibbles 1, 3, 5, 7; v_perm_b32 then builds
// the fp16 pairs 0x64nn64nn = (1024 + n, 1024 + n') from bytes (0, 2) and (1, 3) of each: 7 instructions per dword instead of the
// 11 of shift / and / or per pair.  The integers are exact either way, so the products are the same bits.
__device__ __forceinline__ void dequant_16_i4_perm(const u32x2& w, f16x2 scale2, f16x2 (&out)[8])
{
    const u32   c64      = 0x64646464u;
    const f16x2 bias1032 = {(f16)1032.0f, (f16)1032.0f};
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const u32 wdw = d == 0 ? w.x : w.y;
        const u32 ev  = wdw & 0x0f0f0f0fu;         // nibbles 0, 2, 4, 6 = k-locals 0, 4, 1, 5
        const u32 od  = (wdw >> 4) & 0x0f0f0f0fu;  // nibbles 1, 3, 5, 7 = k-locals 2, 6, 3, 7
        out[4 * d + 0] = (as_f16x2(__builtin_amdgcn_perm(ev, c64, 0x00060004u)) - bias1032) * scale2;  // nibbles 0, 4: k 0, 1
        out[4 * d + 1] = (as_f16x2(__builtin_amdgcn_perm(od, c64, 0x00060004u)) - bias1032) * scale2;  // nibbles 1, 5: k 2, 3
        out[4 * d + 2] = (as_f16x2(__builtin_amdgcn_perm(ev, c64, 0x00070005u)) - bias1032) * scale2;  // nibbles 2, 6: k 4, 5
        out[4 * d + 3] = (as_f16x2(__builtin_amdgcn_perm(od, c64, 0x00070005u)) - bias1032) * scale2;  // nibbles 3, 7: k 6, 7
    }
}

// one step's global loads of one lane: its wave's 16-column group of the weight block (BITS = 8: two 64-k tiles, BITS = 4: one
// 128-k tile) and four dy pieces
template <int BITS>
struct Regs {
    u32x4 wq[BITS == 8 ? 2 : 1];
    u32x4 yq[4];
    f16   sc;
};

// One kernel, two row maps.  GROUPED = false: the plain problem dx[M][K] = dy[M][N] . fp16(q s)^T (eetq_w8a16_gemm_t); the
// trailing arguments are unused.  GROUPED = true (eetq_w8a16_moe_gemm_t, eetq_w4a16_moe_gemm_t): the stack w [E][K][N] (each expert
// the gfx950 layout of its BITS, K * N bytes apart for int8 and K * N / 2 for int4), scales [E][N]; expert e's problem is the contiguous sorted rows offsets[e] .. offsets[e + 1] - 1 of
// dy [S][N] and dx [S][K], M = A = the length of the active list.  The grid is R row-tile slots x ceil(K / 128)
// column tiles, R = floor(S / 128) + min(E, S) >= sum_e ceil(c_e / 128) whatever the routing; slot r is the r-th row tile in the
// order of the active list (ascending experts, padded with -1).  Every wave finds its slot's expert on its own: lane l sums the
// tile counts of active entries l * per .., an inclusive wave scan gives each lane's first tile, and the lane whose range holds
// r hands (expert, first tile) to the others -- no LDS, no barrier; surplus slots exit before any load of the tile.  The tile
// body then runs on the expert's rows with dy, dx and the weight and scale bases moved to them: rows past the expert's count
// read its last row and are never stored.  The GROUPED = false instantiation is the kernel this file had before the grouped map.
//
// BITS = 4 (eetq_w4a16_gemm_t on the plain map, eetq_w4a16_moe_gemm_t on the grouped one): w is the gfx950 int4 layout -- 1 KiB tiles of 16 columns x 128 k ordered
// [n / 16][k / 128], lane ((k >> 5) & 3) * 16 + (n & 15) holds 32 k of one column -- and K % 128 == 0, so a tile's 128 k are ONE
// int4 tile per 16-column group: one 16-byte load per lane and step, no clamped second k tile.
template <bool GROUPED, int BITS>
__global__ __launch_bounds__(256, 2) void gemm_t_kernel(const f16* __restrict__ dy, const uint8_t* __restrict__ w,
                                                        const f16* __restrict__ scales, f16* __restrict__ dx, int M, int N, int K,
                                                        const int* __restrict__ offsets, const int* __restrict__ active, int R)
{
    static_assert(BITS == 8 || BITS == 4, "int8 or int4 tiles");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wk = wave >> 1;

    int m0, k0;
    if constexpr (!GROUPED) {
        const int tiles_m = (M + BM - 1) / BM;
        const int T       = tiles_m * ((K + BK - 1) / BK);
        int       tile;
        {   // each XCD gets a contiguous run of tiles; row tiles fastest, so an XCD's workgroups share weight columns in its L2
            const int b = blockIdx.x, q = T >> 3, r = T & 7, xcd = b & 7, idx = b >> 3;
            tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        }
        m0 = (tile % tiles_m) * BM;
        k0 = (tile / tiles_m) * BK;
    } else {
        const int A = M;
        const int T = R * ((K + BK - 1) / BK);
        int       tile;
        {   // the same XCD order: one expert's row tiles of a column tile share an L2
            const int b = blockIdx.x, q = T >> 3, r = T & 7, xcd = b & 7, idx = b >> 3;
            tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        }
        const int slot = tile % R;
        k0             = (tile / R) * BK;
        const int per  = (A + 63) >> 6;
        int       mine = 0;
        for (int i = 0; i < per; ++i) {
            const int a = lane * per + i;
            const int e = a < A ? active[a] : -1;
            if (e >= 0) mine += (offsets[e + 1] - offsets[e] + BM - 1) / BM;
        }
        int inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        const int first = inc - mine;
        const unsigned long long hit = __ballot(slot >= first && slot < inc);
        if (hit == 0) return;  // beyond the routing's row tiles (the same answer in every wave)
        const int src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(hit));
        int       e = -1, t0 = 0;
        if (lane == src) {  // walk this lane's entries to the one holding the slot
            int t = first;
            for (int i = 0; i < per; ++i) {
                const int a  = lane * per + i;
                const int ea = a < A ? active[a] : -1;
                const int n  = ea >= 0 ? (offsets[ea + 1] - offsets[ea] + BM - 1) / BM : 0;
                if (slot < t + n) {
                    e  = ea;
                    t0 = t;
                    break;
                }
                t += n;
            }
        }
        e  = __builtin_amdgcn_readfirstlane(__shfl(e, src, 64));
        t0 = __builtin_amdgcn_readfirstlane(__shfl(t0, src, 64));
        const int p0 = offsets[e];
        M            = offsets[e + 1] - p0;
        m0           = (slot - t0) * BM;
        dy += (size_t)p0 * N;
        dx += (size_t)p0 * K;
        if constexpr (BITS == 4)  // a compile-time branch: the int8 stride stays the expression it was
            w += (size_t)e * K * N / 2;
        else
            w += (size_t)e * K * N;
        scales += (size_t)e * N;
    }
    constexpr int kTileShift = BITS == 8 ? 6 : 7;  // k per 1 KiB tile: 64 (int8), 128 (int4)
    const int KT = K >> kTileShift, NT = N >> 4;
    const int NS = (N + BN - 1) / BN;

    // ---- global loads: weight tiles (BITS = 8: k tile kt0 + t, clamped: a K % 128 == 64 tail computes columns it never stores;
    // BITS = 4: the one k tile kt0)
    const int    kt0 = k0 >> kTileShift;
    const int    kt1 = kt0 + 1 < KT ? kt0 + 1 : KT - 1;
    const size_t w_lane = (size_t)lane * 16;
    // dy pieces i = 0..3: rows 32 wave + 8 i + lane / 8, 16-byte chunk lane % 8 of the step's 64 columns
    const int yc = lane & 7;
    const f16* yrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int gm  = m0 + 32 * wave + 8 * i + (lane >> 3);
        gm      = gm < M ? gm : M - 1;
        yrow[i] = dy + (size_t)gm * N + 8 * yc;
    }
    auto load = [&](Regs<BITS>& R, int s) {
        int nt = 4 * s + wave;                 // this wave's 16-column group (wave-uniform)
        nt     = nt < NT ? nt : NT - 1;        // beyond N: a valid tile, replaced by zeros when stored
        const uint8_t* wt = w + (size_t)nt * KT * kTileBytes + w_lane;
        R.wq[0] = *reinterpret_cast<const u32x4*>(wt + (size_t)kt0 * kTileBytes);
        if constexpr (BITS == 8) R.wq[1] = *reinterpret_cast<const u32x4*>(wt + (size_t)kt1 * kTileBytes);
        R.sc    = scales[nt * 16 + (lane & 15)];
        const bool yin = s * BN + 8 * yc < N;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            R.yq[i] = yin ? *reinterpret_cast<const u32x4*>(yrow[i] + (size_t)s * BN) : u32x4{0u, 0u, 0u, 0u};
    };

    const int lds0 = (int)(uint32_t)(uintptr_t)(lds_void*)smem;
    // ---- LDS writes of one step: dy rows, and the dequantised weight group as image rows n = 16 wave + lane % 16.  BITS = 8:
    // chunks 8 t + 2 (lane / 16) and the next one (16 k of one column = 32 bytes) of k tile t; BITS = 4: chunks 4 (lane / 16) +
    // 0..3 (32 k of one column = 64 bytes).  Either way w_wr holds the lane's four chunk addresses in ascending k.
    int y_wr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) y_wr[i] = lds0 + y_off(32 * wave + 8 * i + (lane >> 3), yc);
    const int w_row = 16 * wave + (lane & 15);
    int       w_wr[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c)
            w_wr[t][c] = lds0 + Y_BYTES + w_off(w_row, BITS == 8 ? 8 * t + 2 * (lane >> 4) + c : 4 * (lane >> 4) + 2 * t + c);
    auto store = [&](const Regs<BITS>& R, int s, int stage) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *lds16(y_wr[i] + stage) = R.yq[i];
        if (4 * s + wave < NT) {
            const f16x2 sc2 = {R.sc, R.sc};
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f16x2 d[8];
                if constexpr (BITS == 8)
                    dequant_16(R.wq[t], sc2, d);
                else  // dwords (0, 1) then (2, 3) of the lane's one load: k-locals 16 t .. 16 t + 15 in natural order
                    dequant_16_i4_perm(t == 0 ? u32x2{R.wq[0].x, R.wq[0].y} : u32x2{R.wq[0].z, R.wq[0].w}, sc2, d);
                *lds16(w_wr[t][0] + stage) = u32x4{as_u32(d[0]), as_u32(d[1]), as_u32(d[2]), as_u32(d[3])};
                *lds16(w_wr[t][1] + stage) = u32x4{as_u32(d[4]), as_u32(d[5]), as_u32(d[6]), as_u32(d[7])};
            }
        } else {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                *lds16(w_wr[t][0] + stage) = u32x4{0u, 0u, 0u, 0u};
                *lds16(w_wr[t][1] + stage) = u32x4{0u, 0u, 0u, 0u};
            }
        }
    };

    // ---- fragment read addresses.  A (weight, 32 k x 16 n): lane 4q + p of 16-lane group g supplies row n = 8 (g / 2) + 4 r + q
    // of the n sub-step, columns 4p..4p+3 of the 16 k starting at 64 wk + 32 kb + 16 (g % 2); lane i of the group then holds
    // k = that start + i, n = 8 (g / 2) + 4 r + 0..3 -- elements 4r..4r+3 of the 32x32x16 A fragment.  The swizzle key of
    // those rows does not depend on the sub-step (16 rows = whole key periods): sub-step ns is a constant 4 KiB offset.
    const int g = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
    int       a_rd[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 2; ++r)
            a_rd[kb][r] = lds0 + Y_BYTES + w_off(8 * (g >> 1) + 4 * r + qq, 8 * wk + 4 * kb + 2 * (g & 1) + (pp >> 1)) + 8 * (pp & 1);
    // B (dy, 16 n x 32 m): lane holds row m = 64 wm + 32 mb + lane % 32, n = 16 ns + 8 (lane / 32) + 0..7
    int b_rd[2][4];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) b_rd[mb][ns] = lds0 + y_off(64 * wm + 32 * mb + (lane & 31), 2 * ns + (lane >> 5));

    f32x16 acc[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[kb][mb][i] = 0.f;

    auto compute = [&](int stage) {
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) {
            f16x8 a[2], b[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                // EXEC is all ones here: the transposed read gathers across lanes, so no lane-dependent branch may enclose it
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(uint32_t)(a_rd[kb][0] + stage + ns * 4096));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(uint32_t)(a_rd[kb][1] + stage + ns * 4096));
                a[kb] = __builtin_bit_cast(f16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
            }
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) b[mb] = __builtin_bit_cast(f16x8, *lds16(b_rd[mb][ns] + stage));
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
                    acc[kb][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kb], b[mb], acc[kb][mb], 0, 0, 0);
        }
    };

    // ---- pipeline: R[j] holds the loads of the next step it will store; loads run two steps ahead of their compute
    Regs<BITS> r0, r1;
    load(r0, 0);
    if (NS > 1) load(r1, 1);
    store(r0, 0, 0);
    if (NS > 2) load(r0, 2);
    __syncthreads();
    auto iter = [&](int s, Regs<BITS>& R, int cur, int nxt) {
        if (s + 1 < NS) {
            store(R, s + 1, nxt);  // stage nxt was last read by step s - 1, before the previous barrier
            if (s + 3 < NS) load(R, s + 3);
        }
        compute(cur);
        __syncthreads();
    };
    for (int s = 0; s < NS; s += 2) {
        iter(s, r1, 0, STAGE_BYTES);
        if (s + 1 < NS) iter(s + 1, r0, STAGE_BYTES, 0);
    }

    // ---- epilogue: accumulator element 4 q + e of lane l is dx[m = 64 wm + 32 mb + l % 32][k = 64 wk + 32 kb + 8 q + 4 (l / 32) + e]:
    // rounded once to fp16 into a row-major image of the tile (after the last step's barrier), then whole 256-byte rows out
    f16* image = reinterpret_cast<f16*>(smem);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int ml = 64 * wm + 32 * mb + (lane & 31);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int   kl = 64 * wk + 32 * kb + 8 * q + 4 * (lane >> 5);
                const f16x2 lo = {(f16)acc[kb][mb][4 * q + 0], (f16)acc[kb][mb][4 * q + 1]};
                const f16x2 hi = {(f16)acc[kb][mb][4 * q + 2], (f16)acc[kb][mb][4 * q + 3]};
                *reinterpret_cast<u32x2*>(image + ml * kOutRow + kl) = u32x2{as_u32(lo), as_u32(hi)};
            }
        }
    __syncthreads();
    const int c = (tid & 15) * 8;
#pragma unroll
    for (int r0_ = 0; r0_ < BM; r0_ += 16) {
        const int r = r0_ + (tid >> 4);
        const int m = m0 + r;
        if (m < M && k0 + c < K)
            *reinterpret_cast<u32x4*>(dx + (size_t)m * K + k0 + c) = *reinterpret_cast<const u32x4*>(image + r * kOutRow + c);
    }
}

}  // namespace gemm_t
}  // namespace eetq
