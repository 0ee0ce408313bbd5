// The LDS-tiled MFMA dequant-GEMM on ONE int4 weight [K][N / 2]: the prompt path of a W4A16 projection without
// the expansion to int8 tiles.  The kernel is gemm_tile_body (gemm_kernel.hpp) with BITS = 4 and no row map -- gemm.hip's tile
// order, ring, K-half combine, bias / residual epilogue and write-out; only the weight DMA, the weight fragment read and the dequant
// differ (they are moe_int4_tiled.hip's) -- so a row comes out as expand_i4_to_i8_kernel + the unsplit int8 tile make it, bit for
// bit, at either tile shape.  The launcher restates launch_gemm_mfma's plan (gemm.hip) for the int4 byte counts; it owns no scratch,
// allocates nothing and never synchronises.  A file of its own so that the machine code in gemm.o / gemm_splitk.o /
// moe_gemm_tiled.o / moe_int4_tiled.o does not depend on it.
#include "gemm_kernel.hpp"

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

// rows of x one launch may address with 32-bit buffer offsets: below 2 GiB, a multiple of the 128-row tile
int max_rows_of(int K) { return (int)((((1ull << 31) - 1) / ((size_t)K * 2)) / BM * BM); }

// whole 128-deep int4 tiles, at least kMinKSteps + 1 K steps (an even count: the drain that exists is the six-step one), the weight
// and one row tile of x inside the 32-bit buffer offsets; M is unbounded (row chunks)
bool supports(int M, int N, int K)
{
    return M >= 1 && N >= kTileN && N % kTileN == 0 && K % 128 == 0 && K >= 384 && (size_t)N * K / 2 < (1ull << 31) &&
           max_rows_of(K) >= BM;
}

}  // namespace

int launch_gemm_tile_i4(const f16* x, const uint8_t* w, const f16* scales, Epilogue ep, f16* y, int M, int N, int K, int tile_j,
                        hipStream_t stream)
{
    if (!supports(M, N, K) || ep.act != 0) return EETQ_ERR_UNSUPPORTED;  // quiet: the caller runs eetq_w4a16_gemm
    using C1 = TileCfg<1, 2, 4>;
    using C2 = TileCfg<2, 2, 4>;
    const int max_rows = max_rows_of(K);
    const int n_cu     = tile_j == 0 ? device_cu_count() : 1;  // the rule alone asks the device
    // one launch over columns [c0, c0 + cols) of rows [m, m + rows); force_j = 0: the cheaper of the two tile shapes by
    // launch_gemm_mfma's cost rule (a narrow tile costs kNarrow of a wide-tile pass)
    auto launch_cols = [&](int m, int rows, int c0, int cols, int force_j) -> int {
        const int tiles_m = (rows + BM - 1) / BM;
        const int tiles2  = tiles_m * ((cols + C2::BN - 1) / C2::BN);
        const int tiles1  = tiles_m * ((cols + C1::BN - 1) / C1::BN);
        constexpr double kNarrow = 0.70;
        const double cost2 = (double)((tiles2 + n_cu - 1) / n_cu);
        const double cost1 = kNarrow * (double)((tiles1 + n_cu - 1) / n_cu);
        Epilogue     e     = ep;
        if (e.bias) e.bias += c0;
        if (e.residual) e.residual += (size_t)m * N + c0;
        // an int4 tile is 16 columns x 128 k: a tile row of the weight is K / 128 tiles (the int8 layout's is K / 64)
        const uint8_t* wc     = w + (size_t)(c0 / kTileN) * (K / 128) * kTileBytes;
        const bool     narrow = force_j == 1 || (force_j == 0 && cost1 < cost2);
        // > 64 KiB of dynamic LDS: the kernel about to be launched is opted in, once per device (common.hpp)
        static LargeLdsKernel<decltype(&gemm_tile_i4_kernel<2>)> kernels[2] = {{gemm_tile_i4_kernel<2>}, {gemm_tile_i4_kernel<1>}};
        return launch_large_lds(kernels[narrow], "gemm_tile_i4_kernel launch", dim3((unsigned)(narrow ? tiles1 : tiles2)), dim3(256),
                                narrow ? C1::SMEM_BYTES : C2::SMEM_BYTES, stream, x + (size_t)m * K, wc, scales + c0,
                                y + (size_t)m * N + c0, rows, cols, K, N, e);
    };
    for (int m = 0; m < M; m += max_rows) {
        const int rows = M - m < max_rows ? M - m : max_rows;
        if (tile_j != 0) {  // forced shape: the whole problem in one launch per row chunk
            const int st = launch_cols(m, rows, 0, N, tile_j);
            if (st != EETQ_OK) return st;
            continue;
        }
        const int tiles_m = (rows + BM - 1) / BM;
        const int T2      = tiles_m * ((N + C2::BN - 1) / C2::BN);
        // whole rounds of wide tiles, then the ragged last round -- less than half full -- in a second launch (narrow tiles by the
        // cost rule); the int4 tile has no split form, so that round never gets K slices
        const int rem = T2 % n_cu;
        if (T2 > n_cu && rem != 0 && rem * 2 < n_cu && tiles_m <= n_cu) {
            const int cols1 = ((T2 - rem) / tiles_m) * C2::BN;  // columns covered by complete rounds (rounded down)
            if (cols1 > 0 && cols1 < N) {
                int st = launch_cols(m, rows, 0, cols1, 2);
                if (st == EETQ_OK) st = launch_cols(m, rows, cols1, N - cols1, 0);
                if (st != EETQ_OK) return st;
                continue;
            }
        }
        const int st = launch_cols(m, rows, 0, N, 0);
        if (st != EETQ_OK) return st;
    }
    return EETQ_OK;
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
