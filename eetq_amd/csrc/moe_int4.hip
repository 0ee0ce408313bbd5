// Grouped W4A16 GEMM over an [E][K][N / 2] int4 expert stack for decode: the BITS = 4 instantiations of
// moe_gemm_kernel (moe_gemm_kernel.hpp) -- moe.hip's routing tables, grid rule, row loop, gather / contiguous row map and plain /
// glu8 write-out on int4 tiles -- and their plan rule.  A file of its own so that the int8 kernels' machine code in moe.o /
// moe_gemm_tiled.o does not depend on it.
#include <cstdio>

#include "moe_gemm_kernel.hpp"

using namespace eetq;

extern "C" {

int eetq_w4a16_moe_gemm(const void* x, const int8_t* w_packed, const void* scales, const int* offsets, const int* sorted_slot,
                        const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8, void* stream)
{
    const int st = moe_gemm_check("eetq_w4a16_moe_gemm", 4, x, w_packed, scales, offsets, sorted_slot, active, y, T, k, E, N, K, gather,
                                  glu8);
    if (st != EETQ_OK) return st;
    const MoeGemmArgs a = moe_gemm_args(x, w_packed, scales, offsets, sorted_slot, active, y, T, k, E, N, K, gather, glu8, stream);
    const int         KT = K / gemv::Codec<4>::kTileK;  // 128 k per 1 KiB int4 tile (16 columns x 128 k, 32 k per lane)
    // Waves per workgroup x stages in flight per wave, by k tiles (every wave must own >= D of them; an int4 tile is 128 deep).
    // Measured (tools/moe_bench.py --plan-sweep, profiles/r10_moe_int4_plans.jsonl; one MI355X, us per launch, median of 20,
    // uniform routing; "-": fewer than waves x depth k tiles):
    //   projection (k tiles)          T     8x2     8x1     4x2     4x1     6x1     3x2
    //   mixtral gate|up (32)          1     38.2    34.0    33.2    31.9    37.9    33.9
    //                                 4     74.8    64.3    64.8    59.6    71.4    62.0
    //                                 16    139.7   130.4   126.4   123.0   142.8   122.3
    //   mixtral down (112)            1     19.7    19.4    20.3    21.9    21.6    23.4
    //                                 4     34.6    33.5    36.0    33.6    34.8    37.8
    //                                 16    60.9    65.8    65.7    73.2    68.9    69.5
    //   qwen3-30b gate|up (16)        1     11.4    9.2     10.8    7.9     8.1     8.4
    //                                 4     20.2    22.8    21.2    16.6    20.1    20.6
    //                                 16    49.8    47.0    42.8    35.4    45.8    38.2
    //   qwen3-30b down (6)            1     -       -       -       7.5     9.1     9.6
    //                                 4     -       -       -       12.0    14.0    11.8
    //                                 16    -       -       -       23.1    30.2    22.8
    // Up to 32 k tiles four waves with one stage each win or tie everywhere (3 x 2 is 0.2-0.7 us ahead at three points, inside
    // the min - max spread of both); the int8 kernel's 8 x 2 wins only on the deep projection (112 tiles, from T = 16 on; a tie
    // below).  Nothing between 32 and 112 tiles was measured: the rule switches at 64.  Qwen3's down projection (6 tiles) runs on
    // four waves (two of them own two tiles), not on one.  Why the narrow single-stage form wins is not measured (no counter
    // run); the hypothesis is occupancy: at 70 VGPRs six workgroups' waves share a SIMD and hide the latency a second stage
    // would, and a narrow workgroup leaves more column tiles resident per CU.
    // 8 x 1, 4 x 2, 6 x 1 and 3 x 2 existed for that sweep only and were deleted after it (their rows stay in the profile).
    // EETQ_AMD_MOE_I4_PLAN=<waves>x<depth> (behind EETQ_AMD_TUNING=1) forces one of the four instantiations that are left, for
    // A/B runs of the switch point (tools/moe_bench.py --plan-sweep); a plan the shape cannot feed is ignored.
    static const int forced = [] {
        const char* e = tuning_env("EETQ_AMD_MOE_I4_PLAN");
        int         wv = 0, d = 0;
        return e && sscanf(e, "%dx%d", &wv, &d) == 2 ? wv * 16 + d : 0;
    }();
    if (forced && KT >= (forced >> 4) * (forced & 15)) {
        switch (forced) {
            case 8 * 16 + 2: return launch_moe_gemm_inst<4, 8, 2>(a);
            case 4 * 16 + 1: return launch_moe_gemm_inst<4, 4, 1>(a);
            case 2 * 16 + 1: return launch_moe_gemm_inst<4, 2, 1>(a);
            case 1 * 16 + 1: return launch_moe_gemm_inst<4, 1, 1>(a);
            default: break;
        }
    }
    if (KT >= 64) return launch_moe_gemm_inst<4, 8, 2>(a);
    if (KT >= 4) return launch_moe_gemm_inst<4, 4, 1>(a);
    if (KT >= 2) return launch_moe_gemm_inst<4, 2, 1>(a);
    return launch_moe_gemm_inst<4, 1, 1>(a);
}

}  // extern "C"
