// Route-table construction of the routed mixture-of-experts layer as device functions: the two passes of
// moe_route_kernel (moe.hip), shared with the fused router kernel (moe_router.hip), whose finishing workgroup
// builds the same tables from the indices it has just selected.  One workgroup of THREADS threads runs route_tables(); the
// tables depend on the ids alone, never on THREADS or on timing.
#pragma once
#include "common.hpp"

namespace eetq {

// exclusive block-wide prefix sum of v (every thread of the THREADS calls it); *total = the sum over the block.
// wsum: THREADS / 64 ints of LDS.  Deterministic: a fixed tree of integer adds.
template <int THREADS>
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int* total)
{
    constexpr int kWaves = THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int       inc  = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int s = wsum[w];
        base += w < wave ? s : 0;
        all += s;
    }
    __syncthreads();  // wsum is reused by the next call
    *total = all;
    return base + inc - v;
}

// the lanes of this wave whose expert id equals mine (ids < 2^nbits; invalid lanes pass id = -1 and get an empty mask)
__device__ __forceinline__ unsigned long long same_id_lanes(int id, int nbits)
{
    unsigned long long m = __ballot(id >= 0);
    for (int b = 0; b < nbits; ++b) {
        const unsigned long long set = __ballot(id >= 0 && ((id >> b) & 1));
        m &= ((id >> b) & 1) ? set : ~set;
    }
    return id >= 0 ? m : 0ull;
}

// One workgroup of THREADS threads (W = THREADS / 64 waves; wave w owns the w-th contiguous segment of the S slots).
// lds: W * E ints (per-wave, per-expert counters) followed by W ints (scan).  idx(s) = the expert id of slot s (int64).
// Pass 1: wave w counts the ids of its slot segment (the lowest lane of every group of equal ids adds the group's size).
// Scan:   counts, offsets, the active list; every per-wave counter becomes that wave's first position for the expert.
// Pass 2: wave w walks its segment again in the same order: position = its counter + the rank among equal ids of lower lanes.
// Segments are in slot order and so are lanes within a chunk: sorted_slot is ordered by expert, then by slot, whatever the timing.
template <int THREADS, typename IdxFn>
__device__ __forceinline__ void route_tables(IdxFn idx, int S, int E, int A, int* lds, int* __restrict__ counts,
                                             int* __restrict__ offsets, int* __restrict__ sorted_slot, int* __restrict__ position,
                                             int* __restrict__ active)
{
    constexpr int kWaves = THREADS / 64;
    int*      cnt  = lds;               // [kWaves][E]
    int*      wsum = lds + kWaves * E;  // [kWaves]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nbits = 32 - __clz(E - 1 > 0 ? E - 1 : 1);
    for (int i = tid; i < kWaves * E; i += THREADS) cnt[i] = 0;
    __syncthreads();

    const int seg = (S + kWaves - 1) / kWaves;
    const int s0 = wave * seg, s1 = min(S, s0 + seg);
    int*      mine = cnt + wave * E;
    for (int c = s0; c < s1; c += 64) {
        const int     s  = c + lane;
        const int64_t v  = s < s1 ? idx(s) : -1;
        const int     id = (v >= 0 && v < E) ? (int)v : -1;
        const unsigned long long m = same_id_lanes(id, nbits);
        if (id >= 0 && (m & ((1ull << lane) - 1)) == 0) mine[id] += __popcll(m);
    }
    __syncthreads();

    int carry = 0, carry_active = 0;
    for (int e0 = 0; e0 < E; e0 += THREADS) {
        const int e = e0 + tid;
        int       n = 0;
        if (e < E)
            for (int w = 0; w < kWaves; ++w) n += cnt[w * E + e];
        int       tot_n, tot_a;
        const int off = carry + block_excl_scan<THREADS>(n, wsum, &tot_n);
        const int act = carry_active + block_excl_scan<THREADS>(n > 0 ? 1 : 0, wsum, &tot_a);
        if (e < E) {
            counts[e]  = n;
            offsets[e] = off;
            if (n > 0) active[act] = e;
            int base = off;
            for (int w = 0; w < kWaves; ++w) {
                const int c = cnt[w * E + e];
                cnt[w * E + e] = base;
                base += c;
            }
        }
        carry += tot_n;
        carry_active += tot_a;
    }
    if (tid == 0) offsets[E] = carry;
    for (int a = carry_active + tid; a < A; a += THREADS) active[a] = -1;
    for (int s = carry + tid; s < S; s += THREADS) sorted_slot[s] = -1;
    __syncthreads();

    for (int c = s0; c < s1; c += 64) {
        const int     s  = c + lane;
        const int64_t v  = s < s1 ? idx(s) : -1;
        const int     id = (v >= 0 && v < E) ? (int)v : -1;
        const unsigned long long m = same_id_lanes(id, nbits);
        const unsigned long long below = m & ((1ull << lane) - 1);
        int pos = -1;
        if (id >= 0) pos = mine[id] + __popcll(below);  // every lane reads before the group's lowest lane moves the counter on
        if (id >= 0) sorted_slot[pos] = s;
        if (s < s1) position[s] = pos;
        if (id >= 0 && below == 0) mine[id] += __popcll(m);
    }
}

// frees the fused router's hand-over scratch on every device and adds the bytes to *freed (moe_router.hip; eetq_release_workspace)
int release_moe_router_workspace(size_t* freed);

}  // namespace eetq
