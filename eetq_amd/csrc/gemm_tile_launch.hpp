// From a plan (gemm_tile_plan.hpp) to launches of gemm_tile_body's kernels: the walk over row chunks and column segments of the
// dense forms with every pointer and epilogue offset in one place, and the one launch of the grouped forms.  The kernels and
// their LargeLdsKernel tables stay in the .hip file that instantiates them, so no object file depends on another's kernels.
#pragma once
#include "gemm_kernel.hpp"
#include "gemm_tile_plan.hpp"

namespace eetq {

static_assert(tile_plan::kRows == gemm::BM && tile_plan::kStepK == gemm::BK && tile_plan::kMinKSteps == gemm::kMinKSteps &&
                  tile_plan::cols_of(true) == gemm::TileCfg<1>::BN && tile_plan::cols_of(false) == gemm::TileCfg<2>::BN,
              "the plan's tile geometry is the kernel's");
static_assert(tile_plan::lds_bytes(true, 8) == gemm::TileCfg<1>::SMEM_BYTES && tile_plan::lds_bytes(false, 8) == gemm::TileCfg<2>::SMEM_BYTES &&
                  tile_plan::lds_bytes(true, 4) == gemm::TileCfg<1, 2, 4>::SMEM_BYTES && tile_plan::lds_bytes(false, 4) == gemm::TileCfg<2, 2, 4>::SMEM_BYTES,
              "the plan's LDS bytes are the kernel's ring");

// one launch of a dense form: the caller's operands moved to the rows and the columns [seg.c0, seg.c0 + seg.cols) it covers
struct TileLaunch {
    const f16*         x;
    const uint8_t*     w;
    const f16*         scales;
    f16*               y;
    Epilogue           ep;
    int                rows, ldc;
    tile_plan::Segment seg;
};

// launch(TileLaunch) for every launch of the plan of y[M][N] = x[M][K] . w, a weight of `bits`; stops at the first status that is
// not EETQ_OK.  y's row stride is N, or N / 2 under the GLU write-out, whose outputs are half the columns.
template <typename Launch>
inline int for_each_tile_launch(int bits, const f16* x, const uint8_t* w, const f16* scales, const Epilogue& ep, f16* y, int M, int N, int K,
                                int n_cu, int force_j, bool may_slice, Launch&& launch)
{
    const bool glu = ep.act == kActGlu8;
    const int  ldc = glu ? N / 2 : N;
    return tile_plan::for_each_launch(M, N, K, n_cu, force_j, may_slice, [&](int m, int rows, const tile_plan::Segment& s) {
        Epilogue e = ep;
        if (e.bias) e.bias += s.c0;
        if (e.residual) e.residual += (size_t)m * N + s.c0;
        return launch(TileLaunch{x + (size_t)m * K, w + tile_plan::weight_offset(bits, s.c0, K), scales + s.c0,
                                 y + (size_t)m * ldc + (glu ? s.c0 / 2 : s.c0), e, rows, ldc, s});
    });
}

// The grouped forms (moe_gemm_tiled.hip, moe_int4_tiled.hip): one launch of R row-tile slots x column tiles from the
// [narrow][GLU] table; force_j = 1 / 2 names the tile, anything else means the cost rule on the estimated row tiles.
template <int BITS, typename Kern>
inline int launch_grouped_tiles(LargeLdsKernel<Kern> (&kernels)[2][2], const char* what, const f16* x, const uint8_t* w, const f16* scales,
                                const int* offsets, const int* sorted_slot, const int* active, f16* y, int T, int k, int E, int N, int K,
                                bool gather, bool glu8, int force_j, hipStream_t stream)
{
    const gemm::GroupMap map    = gemm::make_group_map(offsets, sorted_slot, active, T, k, E, gather);
    const bool           narrow = force_j == 1 || (force_j != 2 && moe_tiled_narrow(T * k, E, N));
    // > 64 KiB of dynamic LDS: the kernel about to be launched is opted in, once per device (common.hpp)
    return launch_large_lds(kernels[narrow][glu8], what, dim3((unsigned)(map.R * tile_plan::ceil_div(N, tile_plan::cols_of(narrow)))), dim3(256),
                            tile_plan::lds_bytes(narrow, BITS), stream, x, w, scales, y, N, K, glu8 ? N / 2 : N, map);
}

}  // namespace eetq
