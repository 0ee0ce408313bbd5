// The launch plan of the LDS-tiled MFMA GEMM (gemm_tile_body, gemm_kernel.hpp), stated ONCE for its four forms: dense int8
// (gemm.hip), dense int4 (gemm_int4_tiled.hip), grouped int8 (moe_gemm_tiled.hip), grouped int4 (moe_int4_tiled.hip).  Host
// arithmetic only: no HIP call, no environment read, no device query -- the CU count, a forced tile shape and "K slices allowed"
// are arguments -- so a plain C++ program can include it, and eetq_diag_tile_plan shows it to tests/test_tile_plan_cpu.py.
// gemm_tile_launch.hpp turns a plan into launches.
#pragma once
#include <cstddef>

namespace eetq {
namespace tile_plan {

// The tile geometry (gemm_tile_launch.hpp holds these against gemm_kernel.hpp's TileCfg): 128-row tiles, wide = 128 x 128 (J = 2),
// narrow = 128 x 64 (J = 1), 64-deep K steps on a six-stage ring whose unrolled drain needs five of them.
constexpr int kRows = 128, kStepK = 64, kStages = 6, kMinKSteps = kStages - 1;
constexpr int cols_of(bool narrow) { return narrow ? 64 : 128; }
constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
constexpr int row_tiles(int rows) { return ceil_div(rows, kRows); }

// dynamic LDS of one workgroup: the ring's stages of 16 KiB of fp16 activations + the tile's columns of one K step of weights
constexpr int lds_bytes(bool narrow, int bits) { return kStages * (kRows * kStepK * 2 + cols_of(narrow) * kStepK * bits / 8); }

// 128 x 128 tiles are the efficient shape when they fill the chip; 128 x 64 tiles double the workgroup count: they win when the
// wide tiles leave CUs idle (tiles < CUs) or end in a mostly empty round.  Cost in units of one wide-tile pass; a narrow tile
// costs kNarrow of it (measured, profiles/r01_kbench_tile_shapes.txt).  true: the narrow tile is the cheaper one for tiles_m row
// tiles over `cols` columns on n_cu CUs.
inline bool narrow_cheaper(long tiles_m, int cols, long n_cu)
{
    constexpr double kNarrow = 0.70;
    const long t2 = tiles_m * ceil_div(cols, cols_of(false)), t1 = tiles_m * ceil_div(cols, cols_of(true));
    return kNarrow * (double)((t1 + n_cu - 1) / n_cu) < (double)((t2 + n_cu - 1) / n_cu);
}

// The grouped forms: the counts live on the device, so the row tiles are estimated from the shapes -- min(E, S) experts with the
// mean ceil(S / min(E, S)) rows each.
inline long grouped_row_tiles(int S, int E)
{
    const int A = S < E ? S : E;
    return (long)A * row_tiles(ceil_div(S, A));
}

// rows of x one launch may address with 32-bit buffer offsets: below 2 GiB, a multiple of the 128-row tile
inline int max_rows(int K) { return (int)((((1ull << 31) - 1) / ((size_t)K * 2)) / kRows * kRows); }

// the weight lies inside the 32-bit buffer offsets
inline bool weight_fits(int bits, int N, int K) { return (size_t)N * K / (8 / bits) < (1ull << 31); }

// K of the tiled kernel: int8, five K steps (below, launch_gemm_mfma runs the stream kernel); int4, whole 128-deep tiles and at
// least kMinKSteps + 1 K steps (an even count: the drain that exists is the six-step one)
inline bool deep_enough(int bits, int K) { return bits == 4 ? K % 128 == 0 && K >= 384 : K / kStepK >= kMinKSteps; }

// byte offset of column c0 (a multiple of 16) in the weight: tile rows of 16 columns, K / 64 int8 or K / 128 int4 tiles of 1 KiB
inline size_t weight_offset(int bits, int c0, int K) { return (size_t)(c0 / 16) * (K / (bits == 4 ? 128 : 64)) * 1024; }

// one launch over the columns [c0, c0 + cols) of a row chunk; k_slices = 2: the launcher should try two K slices of the narrow
// tile first (it needs the stream's scratch region) and run the segment unsplit, as `narrow` says, when it cannot
struct Segment {
    int  c0, cols;
    bool narrow;
    int  k_slices;
};
constexpr int grid_of(int rows, const Segment& s) { return row_tiles(rows) * ceil_div(s.cols, cols_of(s.narrow)); }

// f(row0, rows) over chunks of at most `chunk` rows, until one returns non-zero
template <typename F>
inline int for_each_row_chunk(int M, int chunk, F&& f)
{
    for (int m = 0; m < M; m += chunk) {
        const int st = f(m, M - m < chunk ? M - m : chunk);
        if (st != 0) return st;
    }
    return 0;
}

// f(segment) over the one or two column segments of a chunk of `rows` rows, until one returns non-zero.  force_j = 1 / 2: that
// shape over all N.  Otherwise the cheaper shape -- or whole rounds of wide tiles, then the ragged last round: when that round
// would be less than half full its columns go to a second launch with the cheaper shape (M = 1024, N = 5120: 320 wide tiles =
// 256 + 64 -> 256 wide + 128 narrow: 73.8 -> ~59 us).  Tile rows of the weight layout are 16 columns, so any multiple of 128
// splits.  The ragged round asks for TWO K slices of the narrow tile when those fill the chip once -- half the loop for ~3.5 us of
// hand-over (M = 1024, N = 5120: 128 narrow tiles -> 256 workgroups of K / 2; K = 13824 164 -> ~135 us) -- where the caller allows
// slicing (int8 under the identity epilogue).
template <typename F>
inline int for_each_segment(int rows, int N, int K, int n_cu, int force_j, bool may_slice, F&& f)
{
    if (force_j != 0) return f(Segment{0, N, force_j == 1, 1});
    const int tiles_m = row_tiles(rows);
    const int T2      = tiles_m * ceil_div(N, cols_of(false));
    const int rem     = T2 % n_cu;
    const int cols1   = ((T2 - rem) / tiles_m) * cols_of(false);  // columns covered by complete rounds (rounded down)
    if (T2 > n_cu && rem != 0 && rem * 2 < n_cu && tiles_m <= n_cu && cols1 > 0 && cols1 < N) {
        const int  rem_tiles = tiles_m * ceil_div(N - cols1, cols_of(true));
        const bool two       = may_slice && rem_tiles * 2 <= n_cu && (K / kStepK) / 2 >= 40;
        const int  st        = f(Segment{0, cols1, false, 1});
        return st != 0 ? st : f(Segment{cols1, N - cols1, narrow_cheaper(tiles_m, N - cols1, n_cu), two ? 2 : 1});
    }
    return f(Segment{0, N, narrow_cheaper(tiles_m, N, n_cu), 1});
}

// f(row0, rows, segment) over every launch of the dense M x N x K problem, in launch order
template <typename F>
inline int for_each_launch(int M, int N, int K, int n_cu, int force_j, bool may_slice, F&& f)
{
    return for_each_row_chunk(M, max_rows(K), [&](int m, int rows) {
        return for_each_segment(rows, N, K, n_cu, force_j, may_slice, [&](const Segment& s) { return f(m, rows, s); });
    });
}

}  // namespace tile_plan
}  // namespace eetq
