// Grouped form of the LDS-tiled MFMA dequant-GEMM over an [E][K][N / 2] int4 expert stack: the prompt path of the
// W4A16 routed experts without the expansion to int8 tiles.  The kernel is gemm_tile_body (gemm_kernel.hpp) with GROUPED and
// BITS = 4 -- moe_gemm_tiled.hip's row map, grid rule, ring, K-half combine and write-outs; only the weight DMA, the weight
// fragment read and the dequant differ -- so a row comes out as eetq_expand_i4_to_i8 + eetq_w8a16_moe_gemm_tiled make it, bit for
// bit, at either tile shape.  The launch is launch_grouped_tiles (gemm_tile_launch.hpp), the int8 form's, with tile_j as the forced
// J; this file supplies the limits and the kernel table.  A file of its own so that the int8 kernels' machine code in gemm.o /
// gemm_splitk.o / moe_gemm_tiled.o does not depend on it.
#include "gemm_tile_launch.hpp"
#include "moe_gemm_kernel.hpp"

namespace eetq {

using namespace gemm;

namespace {

template <int J, bool GLU>
__global__ __launch_bounds__(256, 1) void moe_gemm_tile_i4_kernel(const f16* __restrict__ x, const uint8_t* __restrict__ w,
                                                                  const f16* __restrict__ scales, f16* __restrict__ y, int N, int K,
                                                                  int ldc, GroupMap map)
{
    gemm_tile_body<0, J, false, 2, false, GLU, true, 4>(x, w, scales, y, 0, N, K, ldc, Epilogue{}, 1, nullptr, nullptr, map);
}

// the int8 tile's limits (moe_gemm_tiled_supports) and the int4 layout's: whole 128-deep tiles, and at least kMinKSteps + 1 K steps
// (an even count: the drain that exists is the six-step one)
bool supports(int T, int k, int E, int N, int K, bool gather)
{
    return moe_gemm_tiled_supports(T, k, E, N, K, gather) && K % 128 == 0 && K >= 384;
}

}  // namespace
}  // namespace eetq

using namespace eetq;

extern "C" {

int eetq_w4a16_moe_gemm_tiled(const void* x, const int8_t* w_packed_i4, const void* scales, const int* offsets, const int* sorted_slot,
                              const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8, int tile_j,
                              void* stream)
{
    const int st = moe_gemm_check("eetq_w4a16_moe_gemm_tiled", 4, x, w_packed_i4, scales, offsets, sorted_slot, active, y, T, k, E, N, K,
                                  gather, glu8);
    if (st != EETQ_OK) return st;
    EETQ_REQUIRE(tile_j >= 0 && tile_j <= 2, "eetq_w4a16_moe_gemm_tiled: tile_j is 0 (the launcher's rule), 1 (128 x 64) or 2 (128 x 128)");
    if (!supports(T, k, E, N, K, gather != 0)) return EETQ_ERR_UNSUPPORTED;  // quiet: the caller runs eetq_w4a16_moe_gemm
    // [narrow][GLU]
    static LargeLdsKernel<decltype(&moe_gemm_tile_i4_kernel<2, false>)> kernels[2][2] = {
        {{moe_gemm_tile_i4_kernel<2, false>}, {moe_gemm_tile_i4_kernel<2, true>}},
        {{moe_gemm_tile_i4_kernel<1, false>}, {moe_gemm_tile_i4_kernel<1, true>}}};
    return launch_grouped_tiles<4>(kernels, "moe_gemm_tile_i4_kernel launch", static_cast<const f16*>(x), reinterpret_cast<const uint8_t*>(w_packed_i4),
                                   static_cast<const f16*>(scales), offsets, sorted_slot, active, static_cast<f16*>(y), T, k, E, N, K, gather != 0,
                                   glu8 != 0, tile_j, static_cast<hipStream_t>(stream));
}

int eetq_w4a16_moe_gemm_tiled_supported(int T, int k, int E, int N, int K, int gather)
{
    if (T < 1 || k < 1 || E < 1 || N < 1 || K < 1) return 0;
    return supports(T, k, E, N, K, gather != 0) ? 1 : 0;
}

}  // extern "C"
