// Small-batch (AUTO: 2 <= M <= 16; by explicit path up to 64 rows) W8A16 / W4A16 stream GEMM launcher; kernel in streamk_kernel.hpp.
// Covers the reference's batched-GEMV range (m <= 4, weightOnlyBatchedGemv/kernelLauncher.cu:165-192) and the
// small-M end of its CUTLASS range, where the weight stream -- not the matrix cores -- bounds the time.
//
// One launch = one StreamRecipe.  resolve() is the only place that decides it (the measured rules below, the overrides, every
// clamp); launch_streamk, launch_streamk_i4 and stream_plan_query all call it.  StreamInsts<MT, BITS> lists the kernels that exist,
// one row each; dispatch() walks that list and refuses a recipe that has no row.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <utility>

#include "streamk_kernel.hpp"

namespace eetq {

namespace {

// How a small-batch launch gets its activation fragments: form 0 = registers, 1 = block copy in LDS, 2 = per-wave ring in LDS
// (all three feed the same fragments to the same MFMAs in the same order -- bit-identical results at equal wave count,
// tests/test_gpu_stream_xlds.py):
//   regs  : straight from L2 into registers, 16 (clamped) rows x 128 B per weight tile: two vector loads of activations per vector
//           load of weights (four on int4 tiles), whatever M is
//   block : the M rows copied ONCE per workgroup into LDS (LDS-DMA); needs K % 128 == 0; the per-tile cost is the weight load alone,
//           so one tile row per workgroup is affordable where two load the CUs unevenly
//   ring  : one or more LDS-DMA instructions per k tile and wave into the wave's own ring; any K, no copy up front
struct StreamPlan {
    int form, nt, waves;
};

// The complete launch recipe: the plan, and what follows from it -- the kernel's ring form XM (0 registers, 1 block copy, 2 / 3 / 4 /
// 5 rings of 8 / 4 / 16 / 32 rows), D tiles in flight per wave, OCC = MIN_WAVES_PER_SIMD of its launch bounds.
struct StreamRecipe {
    int form, nt, waves;
    int xm, d, occ;
};

// EETQ_AMD_I{8,4}_STREAM_PLAN=form,nt,waves (rule|regs|block|ring, 1|2, 8|16; "rule" / 0 = as the rule says) overrides single fields
// for A/B runs and tests; _STREAM_WAVES=8 / 16 forces the workgroup size of the register form the rule starts from as well;
// _STREAM_XLDS=0 switches both LDS forms off (the register form with its own tile rows per workgroup and workgroup size: the kernel
// of rounds 1-3).  All empty: the rule alone.
struct StreamOverrides {
    StreamPlan plan{-1, 0, 0};
    int        waves   = 0;
    bool       lds_off = false;
};

// The activation bytes a launch keeps in dynamic LDS NEXT TO the cross-wave reduction area (streamk_smem_bytes): the block copy
// holds M x K fp16, rounded up to 1 KiB; a ring holds 2 D - 1 slots per wave, a slot its rows x one k tile of activations (128 B
// per row on int8 tiles, 256 B on int4 tiles: 1 / 2 / 4 KiB).
constexpr size_t stream_x_lds_bytes(int bits, int xm, int waves, int d, int M, int K)
{
    if (xm == 0) return 0;
    if (xm == 1) return ((size_t)M * K * 2 + 1023) & ~(size_t)1023;
    const int rows = xm == 3 ? 4 : xm == 4 ? 16 : xm == 5 ? 32 : 8;
    return (size_t)waves * (2 * d - 1) * rows * (bits == 8 ? 128 : 256);
}

// The block copy fits only while the SUM of copy and reduction area (WAVES x NT KiB for one row tile) stays within the CU's 160 KiB
// -- for the NT and WAVES the plan actually uses; a plan that does not fit falls back to the register form (same bits).
inline bool block_copy_fits(int bits, int M, int K, int nt, int waves)
{
    return stream_x_lds_bytes(bits, 1, waves, 2, M, K) + streamk::streamk_smem_bytes(1, nt, waves) <= (size_t)kMaxDynamicLds;
}

// The register form's plan.  int8: every workgroup re-reads the activations (M x K fp16 from L2) for its columns; with two tile
// rows per workgroup each activation fragment feeds two weight tiles.  Cost per k tile in wave-load units: NT weight loads + 2
// activation loads, times the workgroups the busiest CU gets.  N = 5120 (320 tile rows on 256 CUs): M = 8 10.0 -> 7.5 us, K = 13824
// 23.6 -> 17.2 us; N = 22016: 24.5 -> 17.0 us; N = 4096 stays at NT = 1 (5.0 vs 5.8 us) -- profiles/r01_kbench_streamk_nt.txt.
// Workgroup size (us with 16 / 8 waves): 5120^2 M = 4 7.59 / 7.08, 13824 x 5120 M = 4 17.03 / 15.26, 5120 x 13824 M = 8 15.69 / 14.67,
// 4096^2 M = 8 5.66 / 5.32; one tile row per workgroup on <= one workgroup per CU at M <= 4 keeps 16 waves (11008 x 4096 M = 2 9.66 / 10.27).
inline StreamPlan regs_plan_i8(int M, int N, int ncu)
{
    int nt = 1;
    if (N % (2 * kTileN) == 0) {
        const long cost1 = (long)((N / kTileN + ncu - 1) / ncu) * 3;
        const long cost2 = (long)((N / (2 * kTileN) + ncu - 1) / ncu) * 4;
        if (cost2 < cost1) nt = 2;
    }
    const int wgs = N / (kTileN * nt);
    return StreamPlan{0, nt, (M > 4 || nt == 2 || wgs > ncu) ? 8 : 16};
}

// int4 (per k tile: NT weight loads + 4 activation loads): 4096 x 11008 M = 4 8.99 -> 8.34 us with 8 waves, 5120 x 13824 10.93 ->
// 10.44, 11008 x 4096 8.46 -> 8.10; N = 5120: 160 two-row workgroups, 5.84 (16 waves) vs 6.29 us
inline StreamPlan regs_plan_i4(int N, int ncu)
{
    int nt = 1;
    if (N % (2 * kTileN) == 0) {
        const long cost1 = (long)((N / kTileN + ncu - 1) / ncu) * 5;
        const long cost2 = (long)((N / (2 * kTileN) + ncu - 1) / ncu) * 6;
        if (cost2 < cost1) nt = 2;
    }
    return StreamPlan{0, nt, N / (kTileN * nt) >= ncu ? 8 : 16};
}

// The rule (int8, one row tile, K / 64 >= 32), read off profiles/r04_stream_plan_sweep.txt (21 shapes x M = 2..8 x 7 plans; "rpc" =
// 16-column tile rows per CU) and checked against the register form of rounds 1-3 in the same run
// (profiles/r04_stream_plan_rule_check.txt, us per launch, registers -> rule; geometric mean over the grid 0.943, worst +1.1 %).
// nt0 / eight0: the register form's tile rows per workgroup and workgroup size.
//   rpc <= 1          ring, 1 row, 16 waves   4096^2 M = 4 5.21 -> 4.71, M = 8 5.33 -> 5.02; 11008 x 4096 M = 4 10.07 -> 8.97;
//                                             8192 x 1024 M = 4 7.04 -> 5.79, M = 8 7.51 -> 6.71; 4096 x 1024 M = 8 4.82 -> 4.21
//   1 < rpc <= 2      registers               (5120^2, 13824 x 5120, 6144^2, 7168^2, 28672 x 8192: nothing beats them by > 2 %)
//                     except N = 32 * CUs (rpc = 2) with K <= 8192 at M <= 5: ring, 1 row, 8 waves (8192^2 M = 4 12.73 -> 11.96)
//                     and M = 2 on rpc <= 1.5: block copy, 1 row (5120^2 7.07 -> 6.74)
//   2 < rpc <= 3      block copy, 1 row, while M*K*2 <= 24 KiB (4096 x 11008 M = 2 10.91 -> 8.94; 3072 x 9216 M = 2 8.43 -> 6.77),
//                     then ring, 1 row, 16 waves (4096 x 11008 M = 4 11.10 -> 9.28, M = 6 11.19 -> 9.65, M = 8 11.41 -> 10.22; 4096 x
//                     12288 M = 4 11.31 -> 9.84; the block copy falls off a cliff once its LDS leaves two workgroups per CU: M = 6 11.64)
//   3 < rpc <= 4      ring, 2 rows, 8 waves   5120 x 13824 M = 4 14.16 -> 13.36, M = 8 14.97 -> 14.21; 4096 x 14336 M = 8 11.96 -> 11.60
//   rpc > 4           ring, 1 row, 16 waves while M <= max(4, K / 1024 - 1), else 2 rows, 8 waves
//                                             8192 x 28672 M = 2 40.5 -> 35.0, M = 4 40.7 -> 35.9; 5120 x 27648 M = 4 24.8 -> 23.7,
//                                             M = 8 27.6 -> 25.7; 4096 x 22016 M = 8 16.77 -> 16.27
// 9 <= M <= 16 (profiles/r04_stream_plan_sweep_m9to16.txt; the ring holds 16 rows, two DMAs per tile):
//   rpc <= 1          ring, 1 row, 16 waves to M = 11, 8 waves from M = 12   4096^2 M = 16 6.38 -> 5.86; 8192 x 1024 M = 16 10.1 -> 8.44;
//                                                                            11008 x 4096 M = 16 13.9 -> 12.6
//   1 < rpc <= 2      ring, 2 rows, 8 waves from M = 12 (5120^2 M = 16 9.79 -> 8.97; 13824 x 5120 M = 16 21.4 -> 19.5), registers below
//   rpc > 2           ring, 2 rows, 8 waves    4096 x 11008 M = 12 12.33 -> 11.74, M = 16 13.45 -> 12.39; 5120 x 13824 M = 16 18.5 -> 16.5;
//                                              8192 x 28672 M = 16 51.5 -> 44.9
// All forms are bit-identical at equal wave count, so a wrong pick costs time only.
inline StreamPlan pick_plan(int M, int N, int K, int ncu, int nt0, bool eight0, bool lds_off)
{
    StreamPlan p{0, nt0, eight0 ? 8 : 16};
    if (lds_off || M > 16) return p;
    const int  rows   = N / kTileN;
    const long xbytes = (long)M * K * 2;
    if (M > 8) {
        if (rows <= ncu) return StreamPlan{2, 1, M >= 12 ? 8 : 16};
        if (N % (2 * kTileN) != 0 || (rows <= 2 * ncu && M < 12)) return p;
        return StreamPlan{2, 2, 8};
    }
    if (rows <= ncu) return StreamPlan{2, 1, 16};
    if (rows <= 2 * ncu) {
        if (rows == 2 * ncu && K <= 8192 && M <= 5) return StreamPlan{2, 1, 8};
        // two rows on up to 1.5 tile rows per CU, K <= 6144: the block copy with one tile row per workgroup (5120^2 7.04 -> 6.73, 4096 x
        // 5120 6.05 -> 5.78, 4096 x 6144 6.35 -> 6.21; deeper K within +-1 %: 13824 x 5120 15.17 / 15.33; not at 1.75 rows per CU:
        // 7168^2 9.78 -> 10.16; not from M = 3)
        if (M == 2 && 2 * rows <= 3 * ncu && K <= 6144 && K % 128 == 0) return StreamPlan{1, 1, 8};
        return p;
    }
    if (rows <= 3 * ncu) return (K % 128 == 0 && xbytes <= 24 * 1024) ? StreamPlan{1, 1, 8} : StreamPlan{2, 1, 16};
    if (rows <= 4 * ncu) return N % (2 * kTileN) == 0 ? StreamPlan{2, 2, 8} : StreamPlan{2, 1, 16};
    // (round 5: at least up to M = 4 whatever K is -- held-out shapes, tools/experiments/stream_plan_sweep.py, profiles/r05_stream_plan_heldout.jsonl:
    // 3584 x 18944 M = 4 ring,1,16 12.69 vs ring,2,8 13.65 us; 4096 x 28672 M = 4 19.88 vs 20.50; costs 4096 x 22016 M = 4 16.02 vs 15.88)
    const int m_one_row = K / 1024 - 1 > 4 ? K / 1024 - 1 : 4;
    return (M <= m_one_row || N % (2 * kTileN) != 0) ? StreamPlan{2, 1, 16} : StreamPlan{2, 2, 8};
}

// W4A16 (K / 128 >= 32, i.e. K >= 4096), read off profiles/r04_stream_plan_sweep_i4.txt and checked against the register form in
// the same run (profiles/r04_stream_plan_rule_check_i4.txt, us per launch, registers -> rule; geometric mean 0.963 at M <= 8, worst
// +1.6 %).  The register form issues FOUR activation loads per weight load; the ring one DMA per tile at M <= 4, two at M <= 8.
//   rpc <= 1, M <= 8     ring, 1 row, 16 waves   11008 x 4096 M = 4 7.98 -> 6.92; 8192 x 1024 M = 4 6.07 -> 5.02; 4096^2 M = 8 4.73 -> 4.46
//   rpc <= 1, M >= 9     16-row ring (four DMAs per tile), 1 row, 8 waves   11008 x 4096 M = 16 13.35 -> 10.02; 8192 x 1024 9.90 -> 7.22;
//                        4096^2 M = 16 6.09 -> 5.23 (the block copy used before the ring existed: 5.32)
//   1 < rpc <= 2, M >= 9 16-row ring, 2 rows, 8 waves from M = 12 (from M = 9 at K >= 6144): 13824 x 5120 M = 16 19.07 -> 14.95; 8192^2
//                        12.14 -> 10.24; 5120^2 8.63 -> 7.67; 7168^2 11.5 -> 9.5; wider shapes stay on registers (ring 6-27 % slower at
//                        M = 9..12) except M >= 15 at K >= 8192 (8192 x 28672 M = 16 39.7 -> 35.3)
//   1 < rpc <= 2         ring, 2 rows, 16 waves above K = 8192 (13824 x 5120 M = 8 13.68 -> 12.32; 28672 x 8192 M = 4 25.5 -> 23.5)
//   2 < rpc <= 3, K 4096 block copy, 1 row, at M <= 5 (4096 x 11008 M = 2 8.36 -> 6.87, M = 5 8.48 -> 7.64; 4096 x 12288 M = 4 8.45 ->
//                        7.62), ring, 1 row, 8 waves above (M = 8 9.00 -> 8.68)
//   rpc > 4              ring, 1 row, 8 waves at M <= 4 from K = 5120 (5120 x 27648 M = 4 18.28 -> 16.57; 8192 x 28672 25.9 -> 24.5);
//                        ring, 2 rows, 8 waves at M >= 5 from K = 8192 (8192 x 28672 M = 8 27.9 -> 26.9)
// and registers everywhere else (5120^2, 5120 x 13824 / 15360, 4096 x 14336 / 22016, 6144^2 ...: nothing beats them by more than 2-3 %).
inline StreamPlan pick_plan_i4(int M, int N, int K, int ncu, int nt0, bool eight0, bool lds_off)
{
    StreamPlan p{0, nt0, eight0 ? 8 : 16};
    if (lds_off) return p;
    const int  rows   = N / kTileN;
    const bool even   = N % (2 * kTileN) == 0;
    if (M > 8) {  // 16-row ring, 4 KiB slots, 8-wave workgroups (profiles/r04_stream_plan_sweep_i4_m9to16.txt)
        if (rows <= ncu) return StreamPlan{2, 1, 8};
        if (rows <= 2 * ncu) return (even && (M >= 12 || K >= 6144)) ? StreamPlan{2, 2, 8} : p;
        return (even && M >= 15 && K >= 8192) ? StreamPlan{2, 2, 8} : p;
    }
    if (rows <= ncu) return StreamPlan{2, 1, 16};
    if (rows <= 2 * ncu) return K > 8192 ? StreamPlan{2, even ? 2 : 1, 16} : p;
    if (rows <= 3 * ncu) return K > 4096 ? p : M <= 5 ? StreamPlan{1, 1, 8} : StreamPlan{2, 1, 8};
    if (rows <= 4 * ncu) return p;
    if (M <= 4 && K >= 5120) return StreamPlan{2, 1, 8};
    if (M >= 5 && K >= 8192 && even) return StreamPlan{2, 2, 8};
    return p;
}

// 17 <= M <= 32: which form the explicit stream path takes (AUTO sends these batch sizes to the split-K tile; abi.hip)
// Measured on the 14 seam shapes x M in {17, 24, 32} (tools/experiments/stream_ring32_seam.py -> profiles/r06_stream_ring32_seam.jsonl):
// the 32-row ring runs at 0.55 - 0.8 of the register form's time everywhere (4096^2 M = 32 10.1 -> 7.9 us, 5120 x 13824 M = 32
// 45 -> 22), one tile row per workgroup up to one workgroup per CU (N = 4096: 4096^2, 11008 x 4096, 14336 x 4096), two beyond.
// Against the split-K plans AUTO runs at these batch sizes it is ahead by >= 5 % on three points only, all at M = 17 (4096^2
// 7.05 -> 6.43, 4096 x 6144 8.67 -> 8.19, 8192^2 16.5 -> 15.0) and 15 - 37 % behind on the wide / deep shapes: AUTO keeps the
// split-K tile from M = 17 (verdict item 5: fewer than five shapes, shelved as an AUTO choice).
inline StreamPlan ring32_plan(int M, int N, int K, int ncu)
{
    (void)M, (void)K;
    return StreamPlan{2, N / kTileN <= ncu ? 1 : 2, 8};
}

// The one decision: which kernel a launch of M rows on bits-wide tiles takes.  Pure host arithmetic -- no environment, no device.
inline StreamRecipe resolve(int bits, int M, int N, int K, int ncu, const StreamOverrides& ov)
{
    const int mt = (M + 15) / 16;                     // 16-row MFMA tiles
    const int KT = K / (bits == 4 ? 128 : kTileK);    // every wave must own >= D k tiles
    if (KT < 32) {                                    // shallow K: fixed register forms
        if (KT >= 16) return StreamRecipe{0, 1, 8, 0, 2, 2};
        if (KT >= 4) return StreamRecipe{0, 1, 4, 0, 1, 1};
        return StreamRecipe{0, 1, 1, 0, 1, 1};
    }
    // (two tiles in flight per wave is the optimum of the ring forms too: one +4.8 %, three +6 %, four +9 % in geometric mean over
    // the sweep's shapes -- profiles/r04_stream_depth_ab.txt, r04_stream_depth1_ab.txt)
    if (mt > 2) return StreamRecipe{0, 1, 16, 0, 2, 4};  // deliberate parity with the parent: 33 <= M <= 64 has this one deep-K form, no override applies
    StreamPlan p;
    if (mt == 2) {
        // 17 <= M <= 32 (round 6): the 32-row per-wave ring -- four LDS-DMAs per k tile and wave, two MFMA row tiles per weight
        // register tile, 8-wave workgroups (4 KiB slots: 16 waves would need 192 KiB of LDS) -- next to the register form.
        p = ring32_plan(M, N, K, ncu);
    } else if (bits == 8) {
        // the register form's own plan (regs_plan_i8): two tile rows per workgroup where that puts fewer loads on the busiest CU;
        // 8-wave workgroups (round 4, profiles/r04_int8_stream_waves_ab.txt) wherever there are two tile rows per workgroup or more
        // workgroups than CUs, and at M > 4
        const StreamPlan regs = regs_plan_i8(M, N, ncu);
        p = pick_plan(M, N, K, ncu, regs.nt, ov.waves ? ov.waves == 8 : regs.waves == 8, ov.lds_off);
    } else {
        // regs_plan_i4: 8-wave workgroups when there are enough of them to give every CU one (round 4,
        // profiles/r04_int4_stream_waves_ab.txt), 16 waves when two tile rows per workgroup leave fewer workgroups than CUs
        const StreamPlan regs = regs_plan_i4(N, ncu);
        p = pick_plan_i4(M, N, K, ncu, regs.nt, ov.waves ? ov.waves == 8 : regs.waves == 8, ov.lds_off);
    }
    if (ov.plan.form >= 0) p.form = ov.plan.form;
    if (ov.plan.nt) p.nt = ov.plan.nt;
    if (ov.plan.waves) p.waves = ov.plan.waves;
    // deliberate parity with the parent: at 17 <= M <= 32 neither _STREAM_WAVES nor _STREAM_XLDS is applied
    if (ov.waves && mt == 1) p.waves = ov.waves;
    if (p.nt == 2 && N % (2 * kTileN) != 0) p.nt = 1;
    if (mt == 2) {
        // deliberate parity with the parent, all three: the ring runs with 8 waves whatever the plan says; a forced block copy is
        // treated as registers; the register form with 16 waves ignores nt
        if (p.form == 2) return StreamRecipe{2, p.nt, 8, 5, 2, 2};
        if (p.waves == 8) return StreamRecipe{0, p.nt, 8, 0, 2, 2};
        return StreamRecipe{0, 1, 16, 0, 2, 4};
    }
    // one row tile.  int4, 9 <= M <= 16: the 16-row ring has 4 KiB slots, 8-wave workgroups only (16 waves would need 192 KiB of LDS)
    if (bits == 4 && p.form == 2 && M > 8) p.waves = 8;
    // the block copy: 128 KiB of rows at most next to int8 tiles, 144 KiB next to int4 tiles
    if (p.form == 1 && (K % 128 != 0 || (long)M * K * 2 > (bits == 4 ? 144 : 128) * 1024 || !block_copy_fits(bits, M, K, p.nt, p.waves)))
        p.form = 0;
    // ring rows: 8 (one DMA per int8 tile, two per int4 tile), 16 from M = 9 (two / four DMAs), 4 up to M = 4 on int4 tiles (one DMA)
    const int xm = p.form != 2 ? p.form : M > 8 ? 4 : (bits == 4 && M <= 4) ? 3 : 2;
    return StreamRecipe{p.form, p.nt, p.waves, xm, 2, bits == 4 ? 2 : 4};
}

// Read once per process, through tuning_env(): without EETQ_AMD_TUNING=1 every field stays empty.
inline const StreamOverrides& stream_overrides(int bits)
{
    static const auto parse = [](const char* plan, const char* waves, const char* xlds) {
        StreamOverrides ov;
        char            form[16] = {0};
        int             nt = 0, wv = 0;
        if (plan && sscanf(plan, "%15[^,],%d,%d", form, &nt, &wv) >= 1) {
            ov.plan.form  = !strcmp(form, "regs") ? 0 : !strcmp(form, "block") ? 1 : !strcmp(form, "ring") ? 2 : -1;
            ov.plan.nt    = nt == 1 || nt == 2 ? nt : 0;
            ov.plan.waves = wv == 8 || wv == 16 ? wv : 0;
        }
        wv         = waves ? atoi(waves) : 0;
        ov.waves   = wv == 0 ? 0 : wv == 8 ? 8 : 16;  // any value but 8 has always meant 16
        ov.lds_off = xlds && atoi(xlds) == 0;
        return ov;
    };
    static const StreamOverrides i8 = parse(tuning_env("EETQ_AMD_I8_STREAM_PLAN"), tuning_env("EETQ_AMD_I8_STREAM_WAVES"),
                                            tuning_env("EETQ_AMD_I8_STREAM_XLDS"));
    static const StreamOverrides i4 = parse(tuning_env("EETQ_AMD_I4_STREAM_PLAN"), tuning_env("EETQ_AMD_I4_STREAM_WAVES"),
                                            tuning_env("EETQ_AMD_I4_STREAM_XLDS"));
    return bits == 4 ? i4 : i8;
}

struct StreamArgs {
    const f16*     x;
    const uint8_t* w;
    const f16*     scales;
    Epilogue       ep;
    f16*           y;
    int            M, N, K;
    hipStream_t    stream;
};

template <int MT, int NT, int WAVES, int D, int OCC, int BITS, int XM>
int launch_inst(const StreamArgs& a)
{
    auto         kern = streamk::streamk_kernel<MT, NT, WAVES, D, OCC, BITS, XM>;
    const size_t smem = streamk::streamk_smem_bytes(MT, NT, WAVES) + stream_x_lds_bytes(BITS, XM, WAVES, D, a.M, a.K);
    if (smem > 64 * 1024) {
        static std::atomic<unsigned long long> opted{0};
        int st = opt_in_large_lds(kern, opted);
        if (st != EETQ_OK) return st;
    }
    launch_kernel(kern, dim3(a.N / (kTileN * NT)), dim3(WAVES * 64), smem, a.stream, a.x, a.w, a.scales, a.y, a.M, a.N, a.K, a.ep);
    return check_hip(hipGetLastError(), "streamk_kernel launch");
}

// The kernels that exist: one row per instantiation of streamk_kernel<MT, NT, WAVES, D, OCC, BITS, XM>.
struct StreamInst {
    int nt, waves, d, occ, xm;
};
template <int MT, int BITS>
struct StreamInsts;
template <>
struct StreamInsts<1, 8> {
    static constexpr StreamInst rows[] = {
        // NT WAVES D OCC XM
        {1, 16, 2, 4, 0}, {1, 8, 2, 4, 0}, {2, 16, 2, 4, 0}, {2, 8, 2, 4, 0},  // registers
        {1, 16, 2, 4, 1}, {1, 8, 2, 4, 1}, {2, 16, 2, 4, 1}, {2, 8, 2, 4, 1},  // block copy
        {1, 16, 2, 4, 2}, {1, 8, 2, 4, 2}, {2, 16, 2, 4, 2}, {2, 8, 2, 4, 2},  // 8-row ring
        {1, 16, 2, 4, 4}, {1, 8, 2, 4, 4}, {2, 16, 2, 4, 4}, {2, 8, 2, 4, 4},  // 16-row ring: two DMAs per tile
        {1, 8, 2, 2, 0},  {1, 4, 1, 1, 0}, {1, 1, 1, 1, 0},                    // K / 64 < 32
    };
};
template <>
struct StreamInsts<2, 8> {
    static constexpr StreamInst rows[] = {
        {1, 8, 2, 2, 5},  {2, 8, 2, 2, 5},                                     // 32-row ring
        {1, 8, 2, 2, 0},  {2, 8, 2, 2, 0},  {1, 16, 2, 4, 0},                  // registers (the first also at K / 64 < 32)
        {1, 4, 1, 1, 0},  {1, 1, 1, 1, 0},                                     // K / 64 < 32
    };
};
template <int MT>
struct StreamInsts<MT, 8> {  // three and four row tiles
    static constexpr StreamInst rows[] = {{1, 16, 2, 4, 0}, {1, 8, 2, 2, 0}, {1, 4, 1, 1, 0}, {1, 1, 1, 1, 0}};
};
template <>
struct StreamInsts<1, 4> {
    static constexpr StreamInst rows[] = {
        {1, 16, 2, 2, 0}, {1, 8, 2, 2, 0}, {2, 16, 2, 2, 0}, {2, 8, 2, 2, 0},  // registers (the second also at K / 128 < 32)
        {1, 16, 2, 2, 1}, {1, 8, 2, 2, 1}, {2, 16, 2, 2, 1}, {2, 8, 2, 2, 1},  // block copy
        {1, 16, 2, 2, 2}, {1, 8, 2, 2, 2}, {2, 16, 2, 2, 2}, {2, 8, 2, 2, 2},  // 8-row ring: two DMAs per tile
        {1, 16, 2, 2, 3}, {1, 8, 2, 2, 3}, {2, 16, 2, 2, 3}, {2, 8, 2, 2, 3},  // 4-row ring: one DMA per tile
        {1, 8, 2, 2, 4},  {2, 8, 2, 2, 4},                                     // 16-row ring: four DMAs per tile
        {1, 4, 1, 1, 0},  {1, 1, 1, 1, 0},                                     // K / 128 < 32
    };
};

template <int MT, int BITS, size_t... I>
int dispatch(const StreamRecipe& r, const StreamArgs& a, std::index_sequence<I...>)
{
    constexpr auto& rows = StreamInsts<MT, BITS>::rows;
    int             st   = EETQ_OK;
    const bool      hit  = ((r.nt == rows[I].nt && r.waves == rows[I].waves && r.d == rows[I].d && r.occ == rows[I].occ && r.xm == rows[I].xm &&
                       ((st = launch_inst<MT, rows[I].nt, rows[I].waves, rows[I].d, rows[I].occ, BITS, rows[I].xm>(a)), true)) || ...);
    if (hit) return st;
    char msg[160];
    snprintf(msg, sizeof msg, "[eetq_amd] stream-MFMA path: no kernel for W%dA16 M = %d: form %d, nt %d, waves %d, D %d, OCC %d, XM %d", BITS,
             a.M, r.form, r.nt, r.waves, r.d, r.occ, r.xm);
    return fail(EETQ_ERR_UNSUPPORTED, msg);
}

template <int MT, int BITS>
int launch_mt(const StreamArgs& a)
{
    const StreamRecipe r = resolve(BITS, a.M, a.N, a.K, device_cu_count(), stream_overrides(BITS));
    return dispatch<MT, BITS>(r, a, std::make_index_sequence<std::size(StreamInsts<MT, BITS>::rows)>{});
}

}  // namespace

// Which plan a small-batch launch takes (eetq_diag_stream_plan): resolve() with empty overrides, i.e. what a production launch runs.
// Returns 0 and fills form (0 registers, 1 block copy, 2 ring), tile rows per workgroup, waves per workgroup, or -1 when the shape is
// outside the kernel (M > 16 rows of one tile, K not a multiple of the tile depth).
int stream_plan_query(int bits, int M, int N, int K, int ncu, int* form, int* nt, int* waves)
{
    const int tile_k = bits == 4 ? 128 : 64;
    if ((bits != 4 && bits != 8) || M < 1 || M > 16 || N < kTileN || N % kTileN || K < tile_k || K % tile_k || ncu < 1) return -1;
    const StreamRecipe r = resolve(bits, M, N, K, ncu, StreamOverrides{});
    *form  = r.form;
    *nt    = r.nt;
    *waves = r.waves;
    return 0;
}

// W4A16, 1 <= M <= 16 (one row tile): int4 tiles carry 128 k
int launch_streamk_i4(const f16* x, const uint8_t* w, const f16* scales, Epilogue ep, f16* y, int M, int N, int K,
                      hipStream_t stream)
{
    if (M < 1 || M > 16 || K % 128)
        return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] W4A16 stream-MFMA path supports 1 <= M <= 16, K % 128 == 0");
    return launch_mt<1, 4>(StreamArgs{x, w, scales, ep, y, M, N, K, stream});
}

int launch_streamk(const f16* x, const uint8_t* w, const f16* scales, Epilogue ep, f16* y, int M, int N, int K,
                hipStream_t stream)
{
    if (M < 1 || M > kStreamMaxM)
        return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] stream-MFMA path supports 1 <= M <= 64");
    const StreamArgs a{x, w, scales, ep, y, M, N, K, stream};
    switch ((M + 15) / 16) {
        case 1: return launch_mt<1, 8>(a);
        case 2: return launch_mt<2, 8>(a);
        case 3: return launch_mt<3, 8>(a);
        default: return launch_mt<4, 8>(a);
    }
}

}  // namespace eetq
