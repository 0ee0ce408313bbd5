// The LDS-tiled MFMA dequant-GEMM on ONE int4 weight [K][N / 2]: the prompt path of a W4A16 projection without
// the expansion to int8 tiles.  The kernel is gemm_tile_body (gemm_kernel.hpp) with BITS = 4 and no row map -- gemm.hip's tile
// order, ring, K-half combine, bias / residual epilogue and write-out; only the weight DMA, the weight fragment read and the dequant
// differ (they are moe_int4_tiled.hip's) -- so a row comes out as expand_i4_to_i8_kernel + the unsplit int8 tile make it, bit for
// bit, at either tile shape.  The launcher walks launch_gemm_mfma's plan (gemm_tile_plan.hpp, through gemm_tile_launch.hpp) with
// the int4 byte counts and no K slices; it owns no scratch, allocates nothing and never synchronises.  A file of its own so that
// the machine code in gemm.o / gemm_splitk.o / moe_gemm_tiled.o / moe_int4_tiled.o does not depend on it.
#include "gemm_tile_launch.hpp"

namespace eetq {

using namespace gemm;

namespace {

template <int J>
__global__ __launch_bounds__(256, 1) void gemm_tile_i4_kernel(const f16* __restrict__ x, const uint8_t* __restrict__ w,
                                                              const f16* __restrict__ scales, f16* __restrict__ y, int M, int N, int K,
                                                              int ldc, Epilogue ep)
{
    gemm_tile_body<0, J, false, 2, false, false, false, 4>(x, w, scales, y, M, N, K, ldc, ep, 1, nullptr, nullptr);
}

// whole 128-deep int4 tiles and enough K steps (tile_plan::deep_enough), the weight and one row tile of x inside the 32-bit buffer
// offsets; M is unbounded (row chunks)
bool supports(int M, int N, int K)
{
    return M >= 1 && N >= kTileN && N % kTileN == 0 && tile_plan::deep_enough(4, K) && tile_plan::weight_fits(4, N, K) &&
           tile_plan::max_rows(K) >= BM;
}

}  // namespace

int launch_gemm_tile_i4(const f16* x, const uint8_t* w, const f16* scales, Epilogue ep, f16* y, int M, int N, int K, int tile_j,
                        hipStream_t stream)
{
    if (!supports(M, N, K) || ep.act != 0) return EETQ_ERR_UNSUPPORTED;  // quiet: the caller runs eetq_w4a16_gemm
    const int n_cu = tile_j == 0 ? device_cu_count() : 1;                // the rule alone asks the device
    // the int4 tile has no split form, so the ragged round never gets K slices
    return for_each_tile_launch(4, x, w, scales, ep, y, M, N, K, n_cu, tile_j, false, [&](const TileLaunch& t) {
        // > 64 KiB of dynamic LDS: the kernel about to be launched is opted in, once per device (common.hpp)
        static LargeLdsKernel<decltype(&gemm_tile_i4_kernel<2>)> kernels[2] = {{gemm_tile_i4_kernel<2>}, {gemm_tile_i4_kernel<1>}};
        return launch_large_lds(kernels[t.seg.narrow], "gemm_tile_i4_kernel launch", dim3((unsigned)tile_plan::grid_of(t.rows, t.seg)), dim3(256),
                                tile_plan::lds_bytes(t.seg.narrow, 4), stream, t.x, t.w, t.scales, t.y, t.rows, t.seg.cols, K, t.ldc, t.ep);
    });
}

}  // namespace eetq

using namespace eetq;

extern "C" {

int eetq_w4a16_gemm_tiled(const void* x, const int8_t* w_packed_i4, const void* scales, const void* bias, const void* residual,
                          void* y, int M, int N, int K, int tile_j, void* stream)
{
    EETQ_REQUIRE(x && w_packed_i4 && scales && y, "eetq_w4a16_gemm_tiled: null pointer");
    EETQ_REQUIRE(M >= 1 && N >= 1 && K >= 1, "eetq_w4a16_gemm_tiled: invalid GEMM shape");
    EETQ_REQUIRE(K % 128 == 0, "eetq_w4a16_gemm_tiled: int4: k must be a multiple of 128");
    EETQ_REQUIRE(N % 16 == 0, "eetq_w4a16_gemm_tiled: n must be a multiple of 16");
    EETQ_REQUIRE(((uintptr_t)x | (uintptr_t)w_packed_i4 | (uintptr_t)y) % 16 == 0,
                 "eetq_w4a16_gemm_tiled: x, weight and y must be 16-byte aligned");
    EETQ_REQUIRE((uintptr_t)scales % 2 == 0 && (!bias || (uintptr_t)bias % 8 == 0) && (!residual || (uintptr_t)residual % 16 == 0),
                 "eetq_w4a16_gemm_tiled: scales must be 2-byte, bias 8-byte and residual 16-byte aligned");
    EETQ_REQUIRE(tile_j >= 0 && tile_j <= 2, "eetq_w4a16_gemm_tiled: tile_j is 0 (the launcher's rule), 1 (128 x 64) or 2 (128 x 128)");
    Epilogue ep;
    ep.bias     = static_cast<const f16*>(bias);
    ep.residual = static_cast<const f16*>(residual);
    return launch_gemm_tile_i4(static_cast<const f16*>(x), reinterpret_cast<const uint8_t*>(w_packed_i4), static_cast<const f16*>(scales),
                               ep, static_cast<f16*>(y), M, N, K, tile_j, static_cast<hipStream_t>(stream));
}

int eetq_w4a16_gemm_tiled_supported(int M, int N, int K)
{
    if (M < 1 || N < 1 || K < 1) return 0;
    return supports(M, N, K) ? 1 : 0;
}

}  // extern "C"
