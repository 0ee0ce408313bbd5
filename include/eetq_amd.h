/*
 * eetq_amd.h -- C ABI of libeetq_amd.so: the MI355X (gfx950) implementation of EETQ's W8A16 hot path.
 *
 * Every entry point replaces one function of the reference's native boundary (the pybind module
 * `EETQ`, /root/reference/csrc/eetpy.cpp:7-19); the reference interface each one stands in for is cited
 * on the declaration.  Plain pointers and sizes only -- no torch types.  All device pointers refer to
 * the *current* HIP device; `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls
 * are asynchronous with respect to the host unless stated otherwise.
 *
 * Return value: 0 (EETQ_OK) on success, a negative EETQ_ERR_* code otherwise; the message for the most
 * recent failure on the calling thread is available from eetq_last_error().  The Python host layer
 * (eetq_amd/ops.py) turns a non-zero status into RuntimeError, which is what the reference's C++
 * exceptions become through pybind (csrc/utils/cuda_utils.h:40-60).
 */
#ifndef EETQ_AMD_H_
#define EETQ_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    EETQ_OK              = 0,
    EETQ_ERR_INVALID     = -1, /* bad argument (null pointer, unsupported shape, unknown enum) */
    EETQ_ERR_HIP         = -2, /* a HIP runtime call or kernel launch failed */
    EETQ_ERR_UNSUPPORTED = -3  /* valid request this build does not implement */
};

/* Element type of the weight handed to the quantiser and of the scales it returns
 * (reference: symmetric_quantize<half,half> / <float,float>, fpA_intB_gemm_wrapper.cu:78-95). */
enum { EETQ_DTYPE_F16 = 0, EETQ_DTYPE_F32 = 1, EETQ_DTYPE_F64 = 2 /* rotary only */ };

/* Byte layout of an int8 [K][N]-shaped weight tensor.
 *   ROW_MAJOR : raw two's-complement int8, element (k,n) at k*N+n -- the reference's "unprocessed" tensor.
 *   GFX950    : this library's native layout (DESIGN.md "HBM layout"): 1 KiB tiles of 16 columns x 64 k,
 *               uint8 = q+128, k-contiguous per column, dword bytes 1<->2 swapped.  What
 *               eetq_w8a16_gemm consumes.  Requires K % 64 == 0, N % 16 == 0.
 *   SM80      : the reference's processed layout for sm75..sm89 (cutlass_preprocessors.cc:497-534;
 *               ColumnMajorTileInterleave<64,2> + row permute + bias/byte swizzle), i.e. the bytes found
 *               in EETQ checkpoints written on NVIDIA GPUs.  Requires K % 64 == 0, N % 64 == 0. */
enum { EETQ_LAYOUT_ROW_MAJOR = 0, EETQ_LAYOUT_GFX950 = 1, EETQ_LAYOUT_SM80 = 2 };

/* Kernel selection for eetq_w8a16_gemm_ex (tests and tuning).  AUTO is what eetq_w8a16_gemm uses. */
enum { EETQ_PATH_AUTO = 0, EETQ_PATH_GEMV = 1 /* M <= 4 */, EETQ_PATH_MFMA = 2 /* LDS-tiled */, EETQ_PATH_STREAM = 3 /* M <= 64; AUTO uses it for 2..16 */,
       EETQ_PATH_MID = 4 /* M <= 128: 32-column tiles, 256-deep K steps; what AUTO runs for 17..128 under EETQ_AMD_SPLITK=0 */,
       EETQ_PATH_SPLITK = 5 /* W8A16: M <= 1024 -- split-K tiles: K slices with an in-launch deterministic reduction and / or row groups
                               of <= 128 rows (AUTO: 17 <= M <= 128, and the row-group plan on few-tile shapes up to M = 1024); W4A16: M <= 128 */,
       EETQ_PATH_TILESPLIT = 6 /* the LDS-tiled kernel with K slices per 128 x 64 tile (few tiles, deep K); unsplit when that does not apply */ };

/* Activation of the fused bias + activation epilogue (eetq_w8a16_gemm_act).  Reference: ActivationType
 * (csrc/utils/activation_types.h:23-38) as dispatched by CutlassFpAIntBGemmRunner::gemm_bias_act
 * (fpA_intB_gemm/fpA_intB_gemm_template.h:492-537): Relu, Gelu (tanh form), Silu, Identity. */
enum { EETQ_ACT_IDENTITY = 0, EETQ_ACT_RELU = 1, EETQ_ACT_GELU = 2, EETQ_ACT_SILU = 3 };

/* ---- quantise --------------------------------------------------------------------------------------
 * Replaces EETQ.quant_weights -> symmetric_quantize_last_axis_of_tensor
 * (csrc/cutlass_kernels/fpA_intB_gemm_wrapper.cu:28-107) -> ft::symmetric_quantize
 * (csrc/cutlass_kernels/cutlass_preprocessors.cc:581-678).
 * Per column n of the row-major [K][N] weight: s32 = max_k|w| * 2^-7 (fp32); scales[n] = (dtype)s32;
 * q = int8(clamp(round_half_away(w / s32), -128, 127)); bit-exact with the reference, including q = 127
 * for an all-zero column.  q_raw (ROW_MAJOR) and q_packed (in `layout`) may each be NULL.
 * All pointers are DEVICE pointers.  `scales` has dtype `w_dtype` and N elements.
 * Two launches: per-row-block column maxima (plain stores: no atomics, no zero fill), then quantise + pack (every pack
 * workgroup reduces the rows of maxima for its 64 columns).
 * eetq_quantize_i8_ws (ABI revision 2): `workspace` holds `workspace_floats` floats (device).
 *   >= eetq_quantize_workspace_floats(K, N) (= N * ceil(K / 128): one row of partial maxima per 128 weight rows): the
 *      two-launch route above;
 *   >= N: a zero fill + atomicMax maxima launch instead of the partial rows (same bytes out, a few us slower);
 *   <  N: EETQ_ERR_INVALID, nothing is launched.
 *   workspace = NULL: the library uses an internal buffer (one per device, allocated once and grown on demand, freed by
 *   eetq_release_workspace: calls that pass NULL must not overlap on one device -- concurrent streams bring their own
 *   workspace, as both Python bindings do); workspace_floats is ignored then.
 * eetq_quantize_i8 (ABI revision 1, kept): no size argument, and revision 1 documented the workspace as N floats -- a
 *   caller-provided workspace is therefore treated as exactly N floats (the atomicMax route); NULL as above.  Callers that
 *   allocate eetq_quantize_workspace_floats() floats should move to eetq_quantize_i8_ws to get the faster route. */
/* Revision history: 1 = round 1-2; 2 = eetq_quantize_i8_ws (sized workspace), eetq_release_stream_workspace, eetq_w4a16_gemm_ex;
 * 3 = eetq_diag_auto_path, EETQ_PATH_SPLITK accepts M <= 1024 (row groups); 4 = eetq_diag_splitk_plan; 5 =
 * eetq_rotary_neox_kvcache_prefill_f16, eetq_greedy_handover_f16, eetq_w8a16_gemm_glu8 at M > 16; 6 = eetq_prefill_attention_f16
 * (+ _supported); 7 = eetq_w8a16_gemm_t (and, added later within 7, eetq_sample_handover_f16, eetq_w4a16_gemm_t, eetq_w4a16_moe_gemm_t, the *_bounded rotary entries that carry the cos|sin table's row count, eetq_diag_tile_plan, eetq_spec_ngram_draft_i64, eetq_spec_accept_f16, eetq_spec_sample_accept_f16).  Revisions only ADD entry points: a caller built against an older header keeps working. */
#define EETQ_AMD_ABI_VERSION 7
int eetq_abi_version(void);   /* EETQ_AMD_ABI_VERSION of the loaded library */
int eetq_quantize_i8_ws(const void* w, int w_dtype, size_t K, size_t N, int8_t* q_raw, int8_t* q_packed,
                        int layout, void* scales, float* workspace, size_t workspace_floats, void* stream);
int eetq_quantize_i8(const void* w, int w_dtype, size_t K, size_t N, int8_t* q_raw, int8_t* q_packed,
                     int layout, void* scales, float* workspace, void* stream);
size_t eetq_quantize_workspace_floats(size_t K, size_t N);

/* Same operation on HOST buffers (what the reference's CPU function receives): uploads w, runs the HIP
 * kernels, downloads the results and synchronises.  Blocking. */
int eetq_quantize_i8_host(const void* w, int w_dtype, size_t K, size_t N, int8_t* q_raw, int8_t* q_packed,
                          int layout, void* scales);

/* ---- pack / unpack ---------------------------------------------------------------------------------
 * Replaces EETQ.preprocess_weights -> preprocess_weights_cuda (fpA_intB_gemm_wrapper.cu:109-128) ->
 * ft::preprocess_weights_for_mixed_gemm (cutlass_preprocessors.cc:497-534).
 * eetq_pack_i8: ROW_MAJOR int8 [K][N] -> `layout`.  eetq_unpack_i8: `layout` -> ROW_MAJOR (the reference has
 * no inverse; needed to load NVIDIA-written checkpoints).  Device pointers; src != dst. */
int eetq_pack_i8(const int8_t* q_raw, size_t K, size_t N, int8_t* q_packed, int layout, void* stream);
int eetq_unpack_i8(const int8_t* q_packed, size_t K, size_t N, int8_t* q_raw, int layout, void* stream);
/* Host-buffer variants (blocking), mirroring the CPU-tensor contract of preprocess_weights. */
int eetq_pack_i8_host(const int8_t* q_raw, size_t K, size_t N, int8_t* q_packed, int layout);
int eetq_unpack_i8_host(const int8_t* q_packed, size_t K, size_t N, int8_t* q_raw, int layout);

/* ---- fused dequant + GEMM --------------------------------------------------------------------------
 * Replaces EETQ.w8_a16_gemm / w8_a16_gemm_ -> w8_a16_gemm_forward_cuda(_)
 * (fpA_intB_gemm_wrapper.cu:130-202), i.e. weight_only_batched_gemv_launcher
 * (csrc/weightOnlyBatchedGemv/kernelLauncher.cu:122-232) for small M and ft::gemm_fp16_int
 * (csrc/cutlass_kernels/fpA_intB_gemm.cu:21-33) otherwise.
 *   y[m][n] = fp16( sum_k fp32(x[m][k]) * fp32( fp16( q[k][n] * scales[n] ) ) ),  fp32 accumulation.
 * x: fp16 [M][K] row-major; w_packed: GFX950 layout of the [K][N] int8 weight; scales: fp16 [N];
 * y: fp16 [M][N] row-major.  Device pointers, 16-byte aligned.  Requires K % 64 == 0, N % 16 == 0, M >= 1. */
int eetq_w8a16_gemm(const void* x, const int8_t* w_packed, const void* scales, void* y, int M, int N, int K,
                    void* stream);
/* ABI revision 7 (additive): out[M][K] = in[M][N] . fp16(q.s)^T, weight in the gfx950 int8 layout [K][N].
 * The input gradient of the projection above (the reference's EetqLinearMMFunction.backward computes it as grad @ W_deq^T
 * after dequantising W through an identity GEMM, python/eetq/modules/qlinear.py:80-94), without materialising W_deq:
 *   out[m][k] = fp16( sum_n fp32(in[m][n]) * fp32( fp16( q[k][n] * scale[n] ) ) ),  fp32 accumulation, one rounding.
 * in: fp16 [M][N] row-major; weight / scale: exactly as eetq_w8a16_gemm takes them (int8 only); out: fp16 [M][K] row-major.
 * Device pointers, 16-byte aligned.  Requires K % 64 == 0, N % 16 == 0, M >= 1.  Deterministic: one pass over N per output
 * tile, no atomics, so repeated calls give identical bits. */
int eetq_w8a16_gemm_t(const void* in, const void* weight, const void* scale, void* out, int M, int N, int K, void* stream);
/* ABI revision 7 (additive): the same input gradient from an int4 weight, out[M][K] = in[M][N] . fp16(q.s)^T with q in -8..7:
 *   out[m][k] = fp16( sum_n fp32(in[m][n]) * fp32( fp16( q[k][n] * scale[n] ) ) ),  fp32 accumulation, one rounding.
 * in: fp16 [M][N] row-major; weight_i4: the gfx950 int4 layout of the [K][N/2] packed weight, exactly as eetq_w4a16_gemm takes
 * it (1 KiB tiles of 16 columns x 128 k ordered [n/16][k/128], K * N / 2 bytes); scale: fp16 [N]; out: fp16 [M][K] row-major.
 * Device pointers; in, weight_i4 and out 16-byte aligned.  Requires K % 128 == 0, N % 16 == 0, M >= 1; a violation returns
 * EETQ_ERR_INVALID with a message before any launch.  Rows >= M of a larger out are left untouched.  The tile and the order of
 * accumulation are eetq_w8a16_gemm_t's: the result bits equal eetq_w8a16_gemm_t on the same integers held as int8 tiles.
 * Deterministic (one pass over N per output tile, no atomics), no scratch, no allocation, capturable in a graph. */
int eetq_w4a16_gemm_t(const void* in, const void* weight_i4, const void* scale, void* out, int M, int N, int K, void* stream);
/* As above with an explicit kernel path (EETQ_PATH_*); returns EETQ_ERR_UNSUPPORTED when the path cannot
 * run the shape (e.g. GEMV with M > 4, STREAM with M > 64). */
int eetq_w8a16_gemm_ex(const void* x, const int8_t* w_packed, const void* scales, void* y, int M, int N,
                       int K, int path, void* stream);

/* Fused bias epilogue: y = fp16(gemm) + bias, the fp16 add done after the fp16 rounding so the
 * result is bit-identical to the reference's separate `output + bias` (python/eetq/modules/qlinear.py:61), without the
 * extra elementwise kernel.  bias: fp16 [N], 8-byte aligned, or NULL.  `path` as in eetq_w8a16_gemm_ex. */
int eetq_w8a16_gemm_bias(const void* x, const int8_t* w_packed, const void* scales, const void* bias, void* y, int M,
                         int N, int K, int path, void* stream);

/* y = fp16(acc) [+ bias[n]] [+ residual[m][n]]: bias as above, then a residual tensor [M][N] (fp16, row stride N, 8-byte
 * aligned) added in fp16 after it -- bit-identical to a separate elementwise add of the GEMM output.  The reference's
 * counterpart is FT's bias / residual epilogue family (csrc/cutlass_kernels/fpA_intB_gemm.cu:35-97,
 * fpA_intB_gemm_template.h:492-537), which its Python layer never reaches.  `residual` may be `y` itself (in-place
 * accumulate into the residual stream); any other overlap is undefined.  Either pointer may be NULL. */
int eetq_w8a16_gemm_fused(const void* x, const int8_t* w_packed, const void* scales, const void* bias,
                          const void* residual, void* y, int M, int N, int K, int path, void* stream);

/* Bias + activation epilogue: replaces ft::gemm_fp16_int_bias_act (csrc/cutlass_kernels/fpA_intB_gemm.cu:35-62;
 * epilogues cutlass_extensions/.../epilogue_helpers.h:20-71), which the reference compiles but does not bind.
 *   act == EETQ_ACT_IDENTITY: exactly eetq_w8a16_gemm_fused (fp16 bias add after the fp16 rounding);
 *   otherwise               : y = fp16( act( acc + fp32(bias[n]) ) ) -- sum and activation in fp32, one rounding, as the
 *                             CUTLASS LinearCombinationRelu / Silu / Generic<GELU_taylor> epilogues compute it -- and the
 *                             optional residual is then added in fp16.  bias may be NULL. */
int eetq_w8a16_gemm_act(const void* x, const int8_t* w_packed, const void* scales, const void* bias, const void* residual,
                        void* y, int M, int N, int K, int path, int act, void* stream);

/* ---- int4 (W4A16) -----------------------------------------------------------------------------------
 * Replaces the quint4x2 branches of EETQ.quant_weights / preprocess_weights (fpA_intB_gemm_wrapper.cu:41-66,
 * cutlass_preprocessors.cc:360-418, 581-678 with PACKED_INT4_WEIGHT_ONLY) and the Int4b instantiations of the GEMV /
 * GEMM (weightOnlyBatchedGemv/kernel.h:68-116; fpA_intB_gemm.cu with uint4b_t).
 * Per column: s32 = max|w| * 2^-3; q = clamp(round_half_away(w / s32), -8, 7); ROW_MAJOR packing = two values per byte
 * along N (element 2j in the low nibble, 2j+1 in the high nibble), tensor [K][N/2] bytes.  N is the LOGICAL column count.
 * GFX950 layout: 1 KiB tiles of 16 columns x 128 k, unsigned nibbles q + 8.  Requires K % 128 == 0,
 * N % 16 == 0 (GFX950) / K % 64 == 0, N % 64 == 0 (SM80). */
int eetq_quantize_i4(const void* w, int w_dtype, size_t K, size_t N, int8_t* q_raw, int8_t* q_packed, int layout,
                     void* scales, float* workspace, void* stream);
int eetq_pack_i4(const int8_t* q_raw, size_t K, size_t N, int8_t* q_packed, int layout, void* stream);
int eetq_unpack_i4(const int8_t* q_packed, size_t K, size_t N, int8_t* q_raw, int layout, void* stream);
/* y = fp16( sum_k fp32(x) * fp32( fp16( q4[k][n] * scales[n] ) ) ) [+ bias] [+ residual]; w_packed in the GFX950 int4 layout. */
int eetq_w4a16_gemm(const void* x, const int8_t* w_packed, const void* scales, const void* bias, const void* residual,
                    void* y, int M, int N, int K, void* stream);
/* As above with an explicit kernel path: EETQ_PATH_AUTO (M = 1: dot2 GEMV on int4 tiles; 2..16: register-streaming MFMA
 * kernel; 17..128: split-K MFMA tile on int4 tiles; above: nibbles expanded to int8 tiles + the W8A16 kernels),
 * EETQ_PATH_GEMV (M <= 4), EETQ_PATH_STREAM (M <= 16), EETQ_PATH_SPLITK (M <= 128; honours EETQ_AMD_SPLITK_PLAN),
 * EETQ_PATH_MFMA (the expansion route at any M).  Other paths: EETQ_ERR_UNSUPPORTED.  The tiled kernel on the int4 tiles
 * themselves -- prompts without the expansion and its scratch -- is not a path of this entry: eetq_w4a16_gemm_tiled below. */
int eetq_w4a16_gemm_ex(const void* x, const int8_t* w_packed, const void* scales, const void* bias, const void* residual,
                       void* y, int M, int N, int K, int path, void* stream);
/* eetq_w4a16_gemm_tiled: the same product from the LDS-tiled MFMA kernel reading the int4 tiles directly: no
 * expansion to int8 tiles, no library-owned scratch, no allocation and no synchronisation, so any shape it takes can be captured
 * into a HIP graph cold.  A row comes out bit for bit as EETQ_PATH_MFMA's unsplit int8 tile makes it, at either tile shape.
 *   tile_j: 0 = the launcher's rule (128 x 128 or 128 x 64 tiles by the int8 launcher's cost rule; whole rounds of wide tiles and
 *   the ragged last round in a second launch), 1 = 128 x 64, 2 = 128 x 128 (one launch per row chunk).
 *   Argument errors (null x / w / scales / y, M, N or K < 1, K % 128, N % 16, x / w / y not 16-byte aligned, bias not 8-byte or
 *   residual not 16-byte aligned, tile_j outside 0..2): EETQ_ERR_INVALID, nothing launched.  A valid shape outside
 *   eetq_w4a16_gemm_tiled_supported returns EETQ_ERR_UNSUPPORTED without a message: the caller runs eetq_w4a16_gemm. */
int eetq_w4a16_gemm_tiled(const void* x, const int8_t* w_packed_i4, const void* scales, const void* bias, const void* residual,
                          void* y, int M, int N, int K, int tile_j, void* stream);
/* eetq_w4a16_gemm_tiled_supported: 1 where eetq_w4a16_gemm_tiled takes these sizes, else 0: M >= 1, N % 16 == 0, K % 128 == 0,
 * K >= 384 (six K steps: the only drain the int4 tile has), N K / 2 < 2^31 and 128 rows of x below 2 GiB.  M is unbounded: rows
 * go in chunks below 2 GiB.  Host arithmetic on the shapes alone: no device needed. */
int eetq_w4a16_gemm_tiled_supported(int M, int N, int K);

/* ---- side ops --------------------------------------------------------------------------------------
 * Replaces EETQ.layernorm_forward -> layernorm_forward_cuda (csrc/layernorm_kernels/layernorm.cu:98-113):
 * T5/RMS norm, out = clamp_fp16( x * rsqrt(mean(x^2) + eps) * gamma ), fp32 math, fp16 I/O.
 * Launches on `stream` (the reference uses the default stream, layernorm.cu:76).  Any cols > 0 and any alignment: 16-byte
 * accesses are used only when cols % 8 == 0 and x, gamma and out are 16-byte aligned. */
int eetq_rmsnorm_f16(const void* x, const void* gamma, void* out, float eps, int rows, int cols, void* stream);

/* Replaces EETQ.rotary_embedding_neox (csrc/embedding_kernels/pos_encoding_kernels.cu:55-87) for fp16:
 * in-place NeoX rotation of q and k ([tokens][heads][head_size]) by cos_sin_cache[positions[t]]
 * ([max_pos][rot_dim], cos half then sin half), every product/sum rounded to fp16 like the reference. */
int eetq_rotary_neox_f16(const int64_t* positions, void* query, void* key, const void* cos_sin_cache,
                         int tokens, int heads, int head_size, int rot_dim, void* stream);

/* The same entry for every floating type the reference dispatches except bfloat16 (AT_DISPATCH_FLOATING_TYPES_AND2,
 * pos_encoding_kernels.cu:73-86; bf16 is outside this library's scope): dtype = EETQ_DTYPE_F16 / F32 / F64, shared by
 * query, key and cache.  F32 / F64 are plain IEEE products and sums of that type WITHOUT contraction (the reference's float
 * instantiation is whatever nvcc's default FMA contraction makes of `x * cos - y * sin`: agreement within one rounding). */
int eetq_rotary_neox(const int64_t* positions, void* query, void* key, const void* cos_sin_cache, int dtype,
                     int tokens, int heads, int head_size, int rot_dim, void* stream);

/* Same rotation on strided operands (no reference counterpart at the pybind boundary; it is what the reference's
 * EETLlamaAttention, python/eetq/modules/llama_modules.py:94-106, needs to rotate the q and k slices of a fused QKV
 * projection in place): q is [tokens][q_heads][head_size] with q_stride elements between tokens, k likewise with
 * k_heads (< q_heads for grouped-query models) and k_stride. */
int eetq_rotary_neox_strided_f16(const int64_t* positions, void* query, void* key, const void* cos_sin_cache,
                                 int tokens, int q_heads, int k_heads, int head_size, int rot_dim, int q_stride,
                                 int k_stride, void* stream);

/* eetq_rotary_neox and eetq_rotary_neox_strided_f16 with the table's row count (added within ABI revision 7): cos_sin_cache has table_rows
 * rows (> 0, else EETQ_ERR_INVALID).  A token whose position is outside [0, table_rows) has no row in the table: nothing is
 * read for it, its q and k are left UNROTATED, and it is counted once (eetq_decode_dropped_steps).  The three entries above
 * carry no row count: they check no upper bound (a position beyond the table reads whatever lies behind it, like the
 * reference); a negative position is left unrotated and counted by them as well. */
int eetq_rotary_neox_bounded(const int64_t* positions, void* query, void* key, const void* cos_sin_cache, int table_rows,
                             int dtype, int tokens, int heads, int head_size, int rot_dim, void* stream);
int eetq_rotary_neox_strided_bounded_f16(const int64_t* positions, void* query, void* key, const void* cos_sin_cache,
                                         int table_rows, int tokens, int q_heads, int k_heads, int head_size, int rot_dim,
                                         int q_stride, int k_stride, void* stream);

/* Grouped decode GEMV (extension; the reference's launcher takes one problem per call,
 * csrc/weightOnlyBatchedGemv/kernelLauncher.cu:122-232): `count` INDEPENDENT M = 1 problems -- no problem reads what
 * another one writes -- in as few dispatches as possible.  Problems of equal K (a multiple of 64 in [2048, 32768]) share
 * one dispatch per 32 problems: their tile rows form one grid, so the ~1.8 us of launch ramp / first-byte latency / tail
 * a 16 MiB GEMV pays per dispatch is paid once per group and the weight stream is as long as the group is.  Results are
 * bit-identical to `count` eetq_w8a16_gemm_fused calls (same kernel body, same summation order) wherever those take the
 * whole-tile-row GEMV kernel, and within one summation-order difference otherwise.  Problems the grouped kernel cannot
 * take (other K) are launched one by one.  `problems` is a HOST array, read during the call (the pointers inside are
 * device pointers, 16-byte aligned; bias / residual may be NULL); capturable in a HIP graph. */
typedef struct {
    const void*   x;        /* fp16 [K] */
    const int8_t* w_packed; /* GFX950 layout of the [K][N] int8 weight */
    const void*   scales;   /* fp16 [N] */
    void*         y;        /* fp16 [N] */
    const void*   bias;     /* fp16 [N] or NULL */
    const void*   residual; /* fp16 [N] or NULL */
    int           N, K;
} eetq_gemv_problem;
int eetq_w8a16_gemv_grouped(const eetq_gemv_problem* problems, int count, void* stream);

/* RMS-norm -> W8A16 GEMV as one launch, M = 1 (extension): y = fp16(sum_k fp32(xn[k]) * fp32(fp16(q*s))) [+ bias] [+ residual]
 * with xn = eetq_rmsnorm_f16(x, gamma, eps) computed while the activation vector is staged in LDS (same arithmetic; the
 * sum of squares is added in a different order, so xn may differ from the separate op by one fp16 ulp in rare elements). */
int eetq_w8a16_gemv_rmsnorm(const void* x, const void* gamma, float eps, const int8_t* w_packed, const void* scales,
                            const void* bias, const void* residual, void* y, int N, int K, void* stream);

/* Gated-MLP activation -> W8A16 GEMV as one launch, M = 1 (extension): gate_up is one row [gate(K) | up(K)] (16-byte
 * aligned, K % 8 == 0); y = W^T . (silu(gate) * up) [+ bias] [+ residual] with the activation computed while the vector is
 * staged in LDS, in the roundings of eetq_silu_mul_f16. */
int eetq_w8a16_gemv_silu_gated(const void* gate_up, const int8_t* w_packed, const void* scales, const void* bias,
                               const void* residual, void* y, int N, int K, void* stream);

/* Gated-MLP activation on a fused gate|up projection output (extension): out[r][i] = silu(gate_up[r][i]) *
 * gate_up[r][intermediate + i], gate_up [rows][2 * intermediate] dense, intermediate % 8 == 0.  fp32 silu rounded to fp16,
 * then an fp16 multiply.  gate_up and out must be 16-byte aligned (EETQ_ERR_INVALID otherwise; the same for
 * eetq_silu_mul_glu8_f16): the kernels move 16 bytes per access. */
int eetq_silu_mul_f16(const void* gate_up, void* out, int rows, int intermediate, void* stream);

/* Gated MLP with the activation in the projection's epilogue (extension).  "glu8" column order of a fused gate|up weight:
 * columns in groups of 16 = gate columns 8t..8t+7 followed by up columns 8t..8t+7 (scales and bias in the same order), so
 * one 16-column tile holds both operands of 8 outputs.
 *   eetq_w8a16_gemv_glu8: M = 1; y[8t + c] = silu_mul(g, u) with g, u the projection's fp16 outputs (+ bias) for the pair,
 *     i.e. exactly eetq_w8a16_gemm (+ bias) followed by eetq_silu_mul_glu8_f16; y has N / 2 entries; gamma non-NULL adds
 *     the RMS-norm prologue of eetq_w8a16_gemv_rmsnorm.
 *   eetq_silu_mul_glu8_f16: out[r][8t + c] = silu_mul(gate_up[r][16t + c], gate_up[r][16t + 8 + c]) for the M > 1 GEMMs over
 *     such a weight; gate_up [rows][2 * intermediate] dense, intermediate % 8 == 0. */
int eetq_w8a16_gemv_glu8(const void* x, const void* gamma, float eps, const int8_t* w_packed, const void* scales,
                         const void* bias, void* y, int N, int K, void* stream);
/*   eetq_w8a16_gemm_glu8: the same for M > 1 rows (no norm prologue): y [M][N / 2].  2 <= M <= 16 (batched decode): the small-
 *     batch kernel's epilogue.  M > 16 (prompts; since ABI 5): where EETQ_PATH_AUTO runs the plain projection on the unsplit tiled
 *     MFMA kernel (eetq_diag_auto_path: EETQ_PATH_MFMA, or EETQ_PATH_TILESPLIT with one slice), that kernel writes silu_mul of its
 *     fp16 tile image -- the same bits as eetq_w8a16_gemm_act
 *     (+ bias) followed by eetq_silu_mul_glu8_f16, without the [M][N] round trip; any other shape returns EETQ_ERR_UNSUPPORTED
 *     and launches nothing (the caller runs those two). */
int eetq_w8a16_gemm_glu8(const void* x, const int8_t* w_packed, const void* scales, const void* bias, void* y, int M, int N,
                         int K, void* stream);
int eetq_silu_mul_glu8_f16(const void* gate_up, void* out, int rows, int intermediate, void* stream);

/* ---- mixture of experts (extension, additive within ABI revision 7) -------------------------------------
 * The reference has no MoE path: these entries extend its per-weight GEMM (w8_a16_gemm_forward_cuda, fpA_intB_gemm_wrapper.cu:
 * 130-173) and its [E, K, N] quantiser input (fpA_intB_gemm_wrapper.cu:45-66, which quantises expert 0 only; eetq_quantize_i8
 * per expert here) to a routed layer.  T tokens each pick k experts of E; "slot" t*k + j is token t's j-th choice.  All three
 * launch a grid fixed by T, k, E, N, K (never by the routing), synchronise nothing and can be captured in a HIP graph.
 *
 * eetq_moe_route: device tables from top_k_index (int64 [T][k], device).  One launch, one workgroup.
 *   counts [E], offsets [E + 1] (exclusive prefix sum; offsets[E] = slots that take part), sorted_slot [T*k]: the slots ordered
 *   by expert, then by slot index (stable, deterministic), -1 from offsets[E] on; position [T*k]: the inverse (slot -> its
 *   sorted position, -1 for a slot that takes part in nothing); active [min(E, T*k)]: the experts with at least one slot, in
 *   ascending order, padded with -1.  Ids outside [0, E) -- transformers' `expert_idx == num_experts` sentinel, -1 -- take part
 *   in nothing.  int32 outputs, device pointers.  1 <= E <= 1024, 1 <= k <= E, T >= 1, T*k <= 2^30; else EETQ_ERR_INVALID. */
int eetq_moe_route(const int64_t* top_k_index, int T, int k, int E, int* counts, int* offsets, int* sorted_slot, int* position,
                   int* active, void* stream);
/* eetq_w8a16_moe_gemm: grouped W8A16 GEMM over an expert stack: w_packed [E][K][N] int8, each expert in the GFX950 layout
 *   (K*N bytes apart), scales fp16 [E][N].  Workgroup (a, column tile): e = active[a] (exits on -1); rows p = offsets[e] ..
 *   offsets[e+1] - 1 in sorted order, 16 at a time, the expert's weight tile row streamed once per 16 rows.
 *     gather = 1: row p reads x[sorted_slot[p] / k] (x fp16 [T][K]);  gather = 0: row p reads x[p] (x fp16 [T*k][K], sorted).
 *     glu8 = 0: y[p][n] = fp16( sum_k fp32(x) * fp32( fp16(q s) ) ), y fp16 [T*k][N] -- the numerics of eetq_w8a16_gemm;
 *     glu8 = 1: columns in "glu8" order (eetq_w8a16_gemm_glu8), y [T*k][N / 2] = silu_mul of the fp16 column pairs -- bit for bit
 *               the projection followed by eetq_silu_mul_glu8_f16.
 *   Rows of y not in any active expert are not written.  offsets / sorted_slot / active as eetq_moe_route wrote them.  Needs
 *   K % 64 == 0, N % 16 == 0, x / w_packed / y 16-byte aligned, E and k as in eetq_moe_route; else EETQ_ERR_INVALID. */
int eetq_w8a16_moe_gemm(const void* x, const int8_t* w_packed, const void* scales, const int* offsets, const int* sorted_slot,
                        const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8, void* stream);
/* eetq_w8a16_moe_gemm_tiled: the same grouped GEMM on the LDS-tiled MFMA kernel (128 x 128 / 128 x 64 tiles, the kernel of
 *   EETQ_PATH_MFMA), for prompts: the signature, argument checks, error codes and y of eetq_w8a16_moe_gemm.  Grid = (floor(T*k /
 *   128) + min(E, T*k)) row-tile slots x column tiles -- an upper bound on sum_e ceil(count_e / 128) for any routing; a workgroup
 *   maps its slot to (expert, 128-row tile) from offsets / active and leaves at once when the slot is surplus.  No host sync, no
 *   atomics, capturable.  Numerics: per live row y[p][n] = fp16( sum_k fp32(x) * fp32( fp16(q s) ) ), fp32 accumulation in the
 *   tile kernel's K order, one rounding; glu8 = 1 rounds both operands to fp16, then silu_mul (= the plain call followed by
 *   eetq_silu_mul_glu8_f16, bit for bit).  An expert's rows equal eetq_w8a16_gemm_ex(..., EETQ_PATH_MFMA) on its gathered rows bit
 *   for bit wherever that call runs the unsplit tile; a row's bits do not depend on T, on the other tokens' routing or on where
 *   the row lands in its tile.  Rows at or past offsets[E] and rows of inactive experts are never written.
 *   Returns EETQ_ERR_UNSUPPORTED, launching nothing and setting no message, for a shape outside the tile kernel's limits (K < 320,
 *   K*N >= 2^31 per expert, rows(x)*K*2 + 4096 >= 2^31): the caller runs eetq_w8a16_moe_gemm, which is correct at any row count. */
int eetq_w8a16_moe_gemm_tiled(const void* x, const int8_t* w_packed, const void* scales, const int* offsets, const int* sorted_slot,
                              const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8, void* stream);
/* 1 when the process asked for the layer's former host path at T > 16 (EETQ_AMD_TUNING=1 and EETQ_AMD_MOE_HOST=1, read once): an
 *   A/B switch for timing the per-expert AUTO launches against the grouped kernels; 0 in every production process. */
int eetq_diag_moe_host_path(void);
/* eetq_moe_combine_f16: out[t][h] = fp16( sum_{j = 0..k-1, in order} fp32(y[position[t*k + j]][h]) * fp32(weights[t][j]) ),
 *   slots with position -1 adding nothing (a token with none gets 0).  y fp16 [*][H], out fp16 [T][H] (16-byte aligned,
 *   H % 8 == 0), weights [T][k] of w_dtype EETQ_DTYPE_F32 (transformers' router output) or EETQ_DTYPE_F16.  No atomics:
 *   deterministic. */
int eetq_moe_combine_f16(const void* y, const int* position, const void* weights, int w_dtype, void* out, int T, int k, int H,
                         void* stream);

/* ---- int4 expert stacks (extension, additive within ABI revision 7) -----------------------------------------
 * eetq_w4a16_moe_gemm: eetq_w8a16_moe_gemm over an int4 expert stack: w_packed [E][K][N / 2] bytes, each expert the GFX950 int4
 *   layout of its [K][N] weight (1 KiB tiles of 16 columns x 128 k, as eetq_quantize_i4 writes it; K*N/2 bytes apart), scales fp16
 *   [E][N].  The same tables, grid (N / 16 column tiles x min(E, T*k) active slots), row loop (16 rows at a time, any number of
 *   rows per expert), gather / glu8 flags, y and untouched rows as eetq_w8a16_moe_gemm; numerics y[p][n] = fp16( sum_k fp32(x) *
 *   fp32( fp16(q s) ) ) with q in -8 .. 7, fp32 accumulation, one rounding; glu8 = 1 is the plain call followed by
 *   eetq_silu_mul_glu8_f16, bit for bit.  A row's bits do not depend on T, on the other tokens' routing or on its place among the
 *   expert's rows.  Needs K % 128 == 0, N % 16 == 0, x / w_packed / y 16-byte aligned, E and k as in eetq_moe_route; else
 *   EETQ_ERR_INVALID.  The forward only: the backward of the int4 experts is eetq_w4a16_moe_gemm_t (below). */
int eetq_w4a16_moe_gemm(const void* x, const int8_t* w_packed, const void* scales, const int* offsets, const int* sorted_slot,
                        const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8, void* stream);
/* eetq_expand_i4_to_i8: GFX950 int4 tiles -> GFX950 int8 tiles holding the same integers (-8 .. 7), on caller-owned memory: src
 *   bytes_src bytes (a whole number of 1 KiB int4 tiles: one weight [K][N / 2] or a stack of them), dst 2 * bytes_src bytes.  int4
 *   tile t becomes int8 tiles 2t and 2t + 1 of the [n / 16][k / 64] order; columns, and with them the scales and a glu8 column
 *   order, are untouched, so eetq_w8a16_gemm / eetq_w8a16_moe_gemm_tiled on dst with the int4 weight's scales compute what the
 *   W4A16 entries define.  One launch, no scratch of the library's, capturable.  16-byte aligned, non-overlapping device pointers;
 *   else EETQ_ERR_INVALID. */
int eetq_expand_i4_to_i8(const int8_t* src, int8_t* dst, size_t bytes_src, void* stream);

/* eetq_w8a16_moe_gemm_tiled_supported: 1 when eetq_w8a16_moe_gemm_tiled takes a projection of these sizes (its shape limits: the
 *   cases for which it would return EETQ_ERR_UNSUPPORTED), else 0.  Host arithmetic only, no device needed.  Lets a caller that has
 *   to prepare something for the tiled kernel first -- the int4 layer's expansion -- decide before it does. */
int eetq_w8a16_moe_gemm_tiled_supported(int T, int k, int E, int N, int K, int gather);
/* eetq_w4a16_moe_gemm_tiled: eetq_w8a16_moe_gemm_tiled on an int4 expert stack (w_packed_i4 [E][K][N / 2] bytes, as
 *   eetq_w4a16_moe_gemm takes it), read by the tile kernel directly: no expansion, no scratch.  The contract is
 *   eetq_w8a16_moe_gemm_tiled's -- tables, gather, glu8, untouched rows, a grid that depends on the shapes only, capturable, no
 *   allocation, no host sync -- and a live row's bits are those of eetq_expand_i4_to_i8 followed by eetq_w8a16_moe_gemm_tiled
 *   (fp16(q s) with one rounding, the same K order), at either tile shape.
 *   tile_j: 0 = the tile shape eetq_w8a16_moe_gemm_tiled would pick for these sizes, 1 = the 128 x 64 tile, 2 = the 128 x 128
 *   tile; anything else EETQ_ERR_INVALID.  Argument checks as eetq_w4a16_moe_gemm (K % 128 == 0, N % 16 == 0, 16-byte aligned
 *   pointers, ...): EETQ_ERR_INVALID, nothing launched.  A valid shape outside eetq_w4a16_moe_gemm_tiled_supported returns
 *   EETQ_ERR_UNSUPPORTED, launching nothing and setting no message: the caller runs eetq_w4a16_moe_gemm. */
int eetq_w4a16_moe_gemm_tiled(const void* x, const int8_t* w_packed_i4, const void* scales, const int* offsets,
                              const int* sorted_slot, const int* active, void* y, int T, int k, int E, int N, int K, int gather,
                              int glu8, int tile_j, void* stream);
/* eetq_w4a16_moe_gemm_tiled_supported: 1 where eetq_w4a16_moe_gemm_tiled takes a projection of these sizes: the limits of
 *   eetq_w8a16_moe_gemm_tiled_supported with K % 128 == 0 and K >= 384 (an even number of 64-deep K steps, at least six).  Host
 *   arithmetic only, no device needed. */
int eetq_w4a16_moe_gemm_tiled_supported(int T, int k, int E, int N, int K, int gather);

/* ---- mixture-of-experts router (extension, additive within ABI revision 7) -----------------------------------
 * The reference has no MoE path.  These entries replace the forward of transformers' *TopKRouter modules (MixtralTopKRouter,
 * Qwen2MoeTopKRouter, Qwen3MoeTopKRouter, OlmoeTopKRouter: F.linear -> softmax(float) -> topk -> sum -> div (-> .to)), five or six
 * torch launches, and the eetq_moe_route launch behind them.  Numerics (what those modules compute on an fp16 model):
 *   logit[t][e] = fp16( sum_h fp32(x[t][h]) * fp32(w[e][h]) ): fp32 accumulation in a fixed order, one rounding;
 *   selection: the k largest fp16 logits of the row, ties to the lower expert id, in descending order;
 *   scores: p = softmax over all E fp16 logits in fp32, max-subtracted; renorm = 1 divides the k selected p by their sum (added
 *     in selection order); written as w_dtype EETQ_DTYPE_F32, or EETQ_DTYPE_F16 = the rounding of the fp32 result.
 *
 * eetq_moe_router_f16: x fp16 [T][H], w fp16 [E][H] (both 16-byte aligned) -> logits_out fp16 [T][E], top_k_index int64 [T][k],
 *   top_k_weights [T][k] of w_dtype and, unless the five table pointers are all NULL (they are all NULL or all set), the tables
 *   eetq_moe_route builds from top_k_index, bit for bit.  T <= 16: ONE launch -- ceil(E / (4 / wpe)) workgroups (wpe = 4, 2, 1 waves
 *   per expert row for H >= 2048, >= 1024, below) stream the weight and hand their sums to the workgroup that finishes last,
 *   through library-owned scratch (one slot per launch stream and device, created by the first call -- not during a graph capture:
 *   EETQ_ERR_UNSUPPORTED then -- and freed by eetq_release_workspace); deterministic, capturable, no host sync.  T > 16: the logits
 *   kernel per 16 tokens, eetq_moe_topk_f16 and (with tables) eetq_moe_route: three launches, for callers without a GEMM of their own.
 *   1 <= E <= 256, 1 <= k <= min(E, 16), H % 64 == 0, 1 <= T <= 16 * 65535, T*k <= 2^30; E > 256 or k > 16: EETQ_ERR_UNSUPPORTED; anything else
 *   out of range, a null pointer, tables half set, renorm not 0 / 1 or a w_dtype other than the two: EETQ_ERR_INVALID.  Every check
 *   runs before any device work.
 * eetq_moe_topk_f16: the selection and the scores alone, from logits fp16 [T][E]: one wave per token, ceil(T / 4) workgroups, the
 *   device code of the fused launch (the same bits from the same logits).  Limits and errors as above. */
int eetq_moe_router_f16(const void* x, const void* w, int T, int H, int E, int k, int renorm, int w_dtype, void* logits_out,
                        int64_t* top_k_index, void* top_k_weights, int* counts, int* offsets, int* sorted_slot, int* position,
                        int* active, void* stream);
int eetq_moe_topk_f16(const void* logits, int T, int E, int k, int renorm, int w_dtype, int64_t* top_k_index, void* top_k_weights,
                      void* stream);

/* ---- the sigmoid, bias-corrected, group-limited router (extension, additive within ABI revision 7) --------------
 * The forward of transformers' DeepseekV3TopkRouter (source-identical in DeepseekV32, Glm4Moe, Glm4MoeLite, Dots1 and SolarOpen): two
 * fp32 casts, F.linear, sigmoid, bias add, per-group top-2 sums, group top-k, mask, expert top-k, gather, sum, div, mul.  Numerics:
 *   logit[t][e] = sum_h fp32(x[t][h]) * fp32(w[e][h]): fp32 accumulation in eetq_moe_router_f16's fixed order, NOT rounded to fp16;
 *   s = 1 / (1 + exp(-logit)), c = s + fp32(bias[e]) in fp32; bias (e_score_correction_bias [E]) is bias_dtype EETQ_DTYPE_F16 or _F32;
 *   n_group contiguous groups of E / n_group experts score the sum of their two largest c; the topk_group best stay, ties to the lower
 *     group id (n_group = 1: no group limiting);
 *   selection: the k largest c among the experts of the kept groups, ties to the lower expert id, in descending order of c;
 *   weights: s[id_j] (without the bias); renorm = 1 divides by (their sum, added in selection order, + 1e-20); then * scale (the
 *     routed_scaling_factor); written as w_dtype EETQ_DTYPE_F32, or EETQ_DTYPE_F16 = the rounding of the fp32 result.
 *
 * eetq_moe_router_sigmoid_f16: x fp16 [T][H], w fp16 [E][H] (16-byte aligned) -> logits_out_f32 float [T][E], top_k_index, top_k_weights
 *   and the tables, as eetq_moe_router_f16: ONE launch at T <= 16 (the same hand-over scratch and slot), above it the logits kernel
 *   per 16 tokens, eetq_moe_topk_sigmoid_f32 and (with tables) eetq_moe_route.  Limits of eetq_moe_router_f16, and 1 <= n_group <= 64,
 *   E % n_group == 0, E / n_group >= 2 when n_group > 1, 1 <= topk_group <= n_group, k <= topk_group * E / n_group, scale finite.
 *   E > 256, k > 16 or n_group > 64: EETQ_ERR_UNSUPPORTED; anything else out of range, a null pointer, a bias_dtype other than the two:
 *   EETQ_ERR_INVALID.  Every check runs before any device work.
 * eetq_moe_topk_sigmoid_f32: the selection and the weights alone, from logits float [T][E]: one wave per token, the device code of the
 *   fused launch (the same bits from the same logits). */
int eetq_moe_router_sigmoid_f16(const void* x, const void* w, const void* bias, int bias_dtype, int T, int H, int E, int k, int n_group,
                                int topk_group, int renorm, float scale, int w_dtype, void* logits_out_f32, int64_t* top_k_index,
                                void* top_k_weights, int* counts, int* offsets, int* sorted_slot, int* position, int* active,
                                void* stream);
int eetq_moe_topk_sigmoid_f32(const void* logits, const void* bias, int bias_dtype, int T, int E, int k, int n_group, int topk_group,
                              int renorm, float scale, int w_dtype, int64_t* top_k_index, void* top_k_weights, void* stream);

/* ---- mixture-of-experts backward (extension, additive within ABI revision 7) --------------------------------
 * The input and router-weight gradients of the layer above with its int8 weights frozen (no weight gradients), on the tables
 * eetq_moe_route wrote and the sorted rows the forward kept.  Grids fixed by the shapes, no host sync, no atomics: deterministic
 * and capturable.
 *
 * eetq_w8a16_moe_gemm_t: grouped eetq_w8a16_gemm_t over an expert stack w_packed [E][K][N] (each expert the GFX950 layout, K*N bytes
 *   apart), scales fp16 [E][N]: for every expert e, rows p = offsets[e] .. offsets[e+1] - 1 of dy fp16 [T*k][N] give the same
 *   rows of dx fp16 [T*k][K] = dy . fp16(q_e s_e)^T, bit for bit eetq_w8a16_gemm_t on those rows and expert e's weight.  Rows of dx
 *   not in any active expert are not written.  offsets / active as eetq_moe_route wrote them.  Needs K % 64 == 0, N % 16 == 0,
 *   dy / w_packed / dx 16-byte aligned, E and k as in eetq_moe_route; else EETQ_ERR_INVALID. */
int eetq_w8a16_moe_gemm_t(const void* dy, const int8_t* w_packed, const void* scales, const int* offsets, const int* active, void* dx,
                          int T, int k, int E, int N, int K, void* stream);
/* eetq_w4a16_moe_gemm_t: eetq_w8a16_moe_gemm_t on an int4 expert stack (w_packed_i4 [E][K][N / 2] bytes, each expert the GFX950 int4
 *   layout, K*N/2 bytes apart), read straight from the int4 tiles: it replaces eetq_expand_i4_to_i8 of the whole stack followed by
 *   eetq_w8a16_moe_gemm_t, whose result bits it equals on the same integers; per expert it is eetq_w4a16_gemm_t on that expert's rows
 *   and weight, bit for bit.  Same tables, untouched rows, grid rule and argument order.  Needs K % 128 == 0, N % 16 == 0, dy /
 *   w_packed_i4 / dx 16-byte aligned, E and k as in eetq_moe_route; else EETQ_ERR_INVALID, before any launch. */
int eetq_w4a16_moe_gemm_t(const void* dy, const int8_t* w_packed_i4, const void* scales, const int* offsets, const int* active,
                          void* dx, int T, int k, int E, int N, int K, void* stream);
/* eetq_moe_combine_bwd_f16: for every slot t*k + j with p = position[t*k + j] >= 0:
 *   dy[p][h] = fp16( fp32(dout[t][h]) * fp32(weights[t][j]) ),   dw[t][j] = sum_h fp32(dout[t][h]) * fp32(y[p][h]) (fixed order),
 *   and dw[t][j] = 0 for slots with p = -1.  dout fp16 [T][H], y / dy fp16 [*][H] (sorted rows), weights / dw [T][k] of w_dtype
 *   EETQ_DTYPE_F32 or EETQ_DTYPE_F16; dw = NULL skips the router gradient.  H % 8 == 0, dout / y / dy 16-byte aligned. */
int eetq_moe_combine_bwd_f16(const void* dout, const void* y, const int* position, const void* weights, int w_dtype, void* dy,
                             void* dw, int T, int k, int H, void* stream);
/* eetq_silu_mul_glu8_bwd_f16: backward of eetq_silu_mul_glu8_f16.  gate_up [rows][2 * intermediate] in glu8 order (the forward's
 *   input), dh [rows][intermediate] (the gradient of its output), dgate_up [rows][2 * intermediate] in the same glu8 order:
 *   du = fp16(dh * s) with s the forward's fp16 silu(g); dg = fp16( fp32(dh) * fp32(u) * sig * (1 + g (1 - sig)) ), sig = sigmoid(g).
 *   intermediate % 8 == 0, 16-byte aligned pointers. */
int eetq_silu_mul_glu8_bwd_f16(const void* gate_up, const void* dh, void* dgate_up, int rows, int intermediate, void* stream);

/* Decode-step rotary + KV-cache write (extension for the EET attention blocks): one new token per batch row b, rotated
 * by cos_sin_cache[positions[b]]; q [batch][q_heads][head_size] is rotated in place, k is rotated and written to
 * k_cache[b][head][slot][:], v is copied to v_cache[b][head][slot][:] (caches [batch][k_heads][max_positions][head_size]).
 * The cache row is slots[b * slot_stride] (DEVICE int64; slot_stride 0 = one slot for the whole batch, e.g. a static
 * cache's token counter; 1 = per row) or, with slots == NULL, positions[b].  The two differ for left-padded batches:
 * the rotary position counts real tokens, the slot counts cache rows.  Same fp16 arithmetic as eetq_rotary_neox_f16.
 * strides (elements): {q_b, k_b, v_b, cache_b, cache_head, cache_pos}.  Rows whose slot is outside [0, max_positions)
 * are left untouched. */
int eetq_rotary_neox_kvcache_f16(const int64_t* positions, const int64_t* slots, int slot_stride, void* query,
                                 const void* key, const void* value, const void* cos_sin_cache, void* k_cache,
                                 void* v_cache, int batch, int q_heads, int k_heads, int head_size, int rot_dim,
                                 const long* strides, int max_positions, void* stream);

/* Prefill form of the above (extension, ABI 5): `tokens` new tokens per batch row.  Token t of row b -- element b * tokens + t
 * of positions and of query / key / value, which advance by ONE stride per token (a fused QKV projection output [batch][tokens]
 * [(q_heads + 2 k_heads) * head_size]) -- is rotated by cos_sin_cache[positions[b * tokens + t]]; q in place, k into
 * k_cache[b][head][base + t][:], v copied to v_cache[b][head][base + t][:], base = *first_row_dev (DEVICE int64, e.g. a static
 * cache's token counter -- read, not advanced) or, with first_row_dev == NULL, first_row.  Replaces the rotary launch plus
 * the two index_copy launches (and their index arithmetic) of a static cache's update on a prompt.  Same fp16 arithmetic as
 * eetq_rotary_neox_f16.  strides (elements): {q_token, k_token, v_token, cache_b, cache_head, cache_pos}.  Host-known rows
 * must satisfy first_row + tokens <= max_positions (EETQ_ERR_INVALID, nothing launched); tokens whose device-side row falls
 * outside [0, max_positions) are left untouched and counted (eetq_decode_dropped_steps). */
int eetq_rotary_neox_kvcache_prefill_f16(const int64_t* positions, void* query, const void* key, const void* value,
                                         const void* cos_sin_cache, void* k_cache, void* v_cache, int batch, int tokens,
                                         const int64_t* first_row_dev, int first_row, int q_heads, int k_heads, int head_size,
                                         int rot_dim, const long* strides, int max_positions, void* stream);

/* The two entries above with the cos|sin table's row count (added within ABI revision 7; table_rows > 0, else EETQ_ERR_INVALID): a token
 * whose position is >= table_rows is treated exactly like one with a negative position or a cache row outside the cache --
 * nothing is read from the table, q is not rotated, nothing is written to the caches, and the token is counted once
 * (eetq_decode_dropped_steps).  The entries without a row count check no upper bound on the position. */
int eetq_rotary_neox_kvcache_bounded_f16(const int64_t* positions, const int64_t* slots, int slot_stride, void* query,
                                         const void* key, const void* value, const void* cos_sin_cache, int table_rows,
                                         void* k_cache, void* v_cache, int batch, int q_heads, int k_heads, int head_size,
                                         int rot_dim, const long* strides, int max_positions, void* stream);
int eetq_rotary_neox_kvcache_prefill_bounded_f16(const int64_t* positions, void* query, const void* key, const void* value,
                                                 const void* cos_sin_cache, int table_rows, void* k_cache, void* v_cache,
                                                 int batch, int tokens, const int64_t* first_row_dev, int first_row,
                                                 int q_heads, int k_heads, int head_size, int rot_dim, const long* strides,
                                                 int max_positions, void* stream);
/* The two bounded cache-write entries on a RING cache (extension, added within ABI revision 7; "The ring cache" below): the caches
 * hold `ring_rows` rows and the row an entry derives -- slots[..] or the position; *first_row_dev or first_row, plus t -- counts the
 * sequence's tokens without an upper bound and is written at row mod ring_rows.  Only a negative row or a position outside the table
 * drops a token (and counts).  The prefill entry takes at most ring_rows tokens per call (EETQ_ERR_INVALID beyond: a call's rows must
 * not meet themselves).  Everything else as the bounded entries; the bits written are theirs. */
int eetq_rotary_neox_kvcache_ring_f16(const int64_t* positions, const int64_t* slots, int slot_stride, void* query, const void* key,
                                      const void* value, const void* cos_sin_cache, int table_rows, void* k_cache, void* v_cache,
                                      int batch, int q_heads, int k_heads, int head_size, int rot_dim, const long* strides,
                                      int ring_rows, void* stream);
int eetq_rotary_neox_kvcache_prefill_ring_f16(const int64_t* positions, void* query, const void* key, const void* value,
                                              const void* cos_sin_cache, int table_rows, void* k_cache, void* v_cache, int batch,
                                              int tokens, const int64_t* first_row_dev, int first_row, int q_heads, int k_heads,
                                              int head_size, int rot_dim, const long* strides, int ring_rows, void* stream);

/* Greedy decode hand-over (extension, ABI 5; the reference's recipe leaves this to transformers' generate loop,
 * examples/models/llama_transformers_example.py:68-79): for each of `batch` rows of fp16 logits [batch][vocab] (row_stride
 * elements apart) the index of the maximum -- the first one on ties, a NaN counts as the maximum: torch.argmax's answer -- is
 * written to out_tokens[b][*column] ([batch][out_cols] int64, out_stride elements apart; skipped when *column is outside
 * [0, out_cols)) and to next_token[b]; then *position += 1 and *column += 1 (DEVICE int64 scalars).  One launch, capturable:
 * what a HIP-graph decode loop does between two model steps. */
int eetq_greedy_handover_f16(const void* logits, long row_stride, int vocab, int batch, int64_t* out_tokens, long out_stride,
                             int out_cols, int64_t* column, int64_t* next_token, int64_t* position, void* stream);

/* Sampling decode hand-over (extension, added within ABI 7; what transformers' generate does with do_sample=True and an EOS
 * token): the bookkeeping of eetq_greedy_handover_f16 -- token to out_tokens[b][*column] (skipped outside [0, out_cols), still
 * handed on) and next_token[b], then *position += 1 and *column += 1; one launch, capturable, no host sync, no allocation -- with
 * the token of a row chosen by temperature / top-k / top-p sampling.
 *   params : DEVICE block of 32 bytes, 8-byte aligned, read by the kernel (a captured graph serves any setting):
 *            float temperature (0 selects greedy; negative or NaN too), float top_p (>= 1, <= 0 or NaN: off), int32 top_k
 *            (<= 0 or >= vocab: off), int32 eos_token (< 0: none), int32 pad_token, int32 reserved (0), uint64 seed.
 *   done   : DEVICE int32[batch] or NULL.  A row with done[b] != 0 is not sampled: it writes and hands on pad_token.  A row whose
 *            token equals eos_token writes that token and sets done[b] = 1.  NULL: no EOS handling.
 *   uniforms: DEVICE float[batch] in [0, 1) or NULL: the row's random number u.  NULL: u = (x0 >> 8) * 2^-24 with
 *            (x0, x1, x2, x3) = Philox4x32-10(counter = (col_lo, col_hi, b, 0), key = (seed_lo, seed_hi)), col = *column at entry:
 *            no state is kept, and every replay of a captured graph draws afresh because the graph advances the column.
 * The token of a row, deterministic given u:
 *   temperature == 0: the token of eetq_greedy_handover_f16 (first index of the maximum, NaN = maximum).
 *   otherwise: NaN counts as -inf; a maximum of +inf gives the first index holding +inf; nothing above -inf gives index 0;
 *   z_i = float(logit_i) / temperature (order and ties: those of the fp16 logits); top-k (0 < k < vocab) keeps z_i >= the k-th
 *   largest value, ties at the threshold included; top-p (0 < p < 1) walks the distinct values of the survivors in descending
 *   order and keeps a value class iff the softmax mass of the strictly larger classes is < p (a tie is never cut: the whole
 *   class stays); the survivors, ordered by value descending then index ascending and renormalised, are walked until the
 *   cumulative probability exceeds u (none: the last survivor).  fp32 exponentials, integer (fixed-point) sums: every cumulative
 *   sum compared against p or u is within 2^-14 absolute of exact arithmetic.  The token index is always < vocab.
 * EETQ_ERR_INVALID (nothing launched): a null logits / out_tokens / column / next_token / position / params, vocab <= 0,
 * batch < 0 or >= 2^24, row_stride < vocab, out_cols <= 0, out_stride < out_cols, params not 8-byte aligned.  batch == 0: OK, no
 * launch.  One workgroup per row; the row that finishes last does the advance, counted in bits 40.. of *position for the length
 * of the launch: -2^39 <= *position < 2^39 (outside it the counters do not advance), and nothing else may touch *position while
 * the launch runs.  Rows of more than 2^23 entries are summed in 2^-32 instead of 2^-40 steps. */
int eetq_sample_handover_f16(const void* logits, long row_stride, int vocab, int batch, int64_t* out_tokens, long out_stride,
                             int out_cols, int64_t* column, int64_t* next_token, int64_t* position, const void* params,
                             int32_t* done, const float* uniforms, void* stream);

/* Speculative greedy decoding by n-gram lookup (extension, added within ABI 7; what transformers' generate does with
 * prompt_lookup_num_tokens): a draft of k tokens from the sequence's own history, and the hand-over of a verify pass over
 * k + 1 rows.  Both are one launch each, capturable, no host sync, no allocation, no atomics: deterministic.
 *
 * eetq_spec_ngram_draft_i64: hist is int64 [batch][cols] (hist_stride elements apart), *position a DEVICE int64.  Per row,
 * L = clamp(*position + 1, 1, cols); hist[b][0 .. L-1] are the row's tokens, the last one the pending token.  For
 * n = min(max_ngram, L - 1) down to 1: the LARGEST e in [n - 1, L - 2] with hist[e-n+1 .. e] == hist[L-n .. L-1]; the first n
 * with a hit wins (the longest match, the most recent among equals).  Then draft[b][i] = ext[e + 1 + i], i < k, where ext is
 * hist[b][0 .. L-1] followed by the draft itself (a match that runs off the end continues into its own draft: a period-p
 * repetition keeps cycling).  No hit: every draft[b][i] = hist[b][L-1].  draft is int64 [batch][k], draft_stride apart.
 * EETQ_ERR_INVALID (nothing launched): a null hist / position / draft, max_ngram outside 1 .. 8, k outside 1 .. 15,
 * batch <= 0, cols <= 0, hist_stride < cols, draft_stride < k, a pointer that is not 8-byte aligned. */
int eetq_spec_ngram_draft_i64(const int64_t* hist, long hist_stride, int cols, int batch, const int64_t* position, int max_ngram,
                              int k, int64_t* draft, long draft_stride, void* stream);

/* eetq_spec_accept_f16: logits is fp16 [batch][k + 1][vocab] (stride_b / stride_t elements apart, vocab dense, any alignment
 * of the rows), the verify pass over [pending token | draft].  g[b][t] = the argmax of logits[b][t] by
 * eetq_greedy_handover_f16's rule (first index of the maximum, NaN = maximum, -0 == +0).  a_b = the number of leading t < k
 * with draft[b][t] == g[b][t]; n = min over b of a_b (the rows share one cache counter and advance together);
 * adv = clamp(min(n + 1, *limit - *column), 0, k + 1).  For j < adv, g[b][j] is written to out_tokens[b][*column + j]
 * ([batch][out_cols], out_stride apart) and to hist[b][*position + 1 + j] ([batch][hist_cols], hist_stride apart), columns
 * outside the arrays skipped; with adv > 0, next_token[b * next_stride] = g[b][adv - 1].  Then *position += adv,
 * *column += adv, stats[0] += 1, stats[1] += adv (DEVICE int64 scalars; stats is int64[2]: verify steps, tokens).  With
 * adv == 0 only stats[0] moves.  One workgroup walks the rows position by position and stops behind the first position a row
 * rejects: a rejected draft reads batch rows of logits, an accepted one batch * (k + 1).
 * EETQ_ERR_INVALID (nothing launched): a null pointer, k outside 1 .. 15, vocab <= 0, batch <= 0, stride_t or stride_b < vocab,
 * draft_stride < k, out_cols <= 0, out_stride < out_cols, hist_cols <= 0, hist_stride < hist_cols, next_stride < 1, an int64
 * pointer that is not 8-byte aligned, logits not 2-byte aligned. */
int eetq_spec_accept_f16(const void* logits, long stride_b, long stride_t, int vocab, int batch, int k, const int64_t* draft,
                         long draft_stride, int64_t* out_tokens, long out_stride, int out_cols, int64_t* column, int64_t* position,
                         const int64_t* limit, int64_t* next_token, long next_stride, int64_t* hist, long hist_stride,
                         int hist_cols, int64_t* stats, void* stream);

/* Speculative decoding for SAMPLED generation (extension, added within ABI 7; what transformers' generate does
 * with prompt_lookup_num_tokens and do_sample=True): eetq_spec_accept_f16 with every token drawn as eetq_sample_handover_f16
 * draws it.  A draft token is a point mass, so exact speculative sampling is: draw x from the target distribution, accept iff
 * x == draft, hand x over either way.  The first 20 arguments are those of eetq_spec_accept_f16, in its order and meaning; then
 *   params  : the 32-byte DEVICE block of eetq_sample_handover_f16, 8-byte aligned.
 *   done    : DEVICE int32[batch] or NULL, the rows' EOS flags.
 *   uniforms: DEVICE float [batch][k + 1] (uniforms_stride elements apart) or NULL: the random numbers, instead of the kernel's own.
 *   workspace: DEVICE int64[batch * (k + 1)], 8-byte aligned; contents irrelevant at entry, undefined afterwards.
 * With col = *column, pos = *position, want = clamp(*limit - col, 0, k + 1):
 * 1. Draw.  For every b and t < want, x[b][t] is the token eetq_sample_handover_f16 produces for the row logits[b][t] with the
 *    same params at column col + t for row b: the greedy rule when temperature is <= 0 or NaN; otherwise u from Philox counter
 *    (lo(col + t), hi(col + t), b, 0) keyed by the seed, or uniforms[b][t] clamped as that entry clamps it; the same NaN, +-inf,
 *    tie, top-k and top-p rules.  Positions >= want are not read.
 * 2. Walk t = 0 .. want - 1 with fin_b = (done[b] != 0) at entry (0 where done is NULL): y[b][t] = pad_token if fin_b, else
 *    x[b][t]; if eos_token >= 0 and y[b][t] == eos_token, fin_b becomes 1.  Row b OBJECTS at t iff t < k, it is not fin_b after this
 *    position, and draft[b][t] != y[b][t] (a finished row never objects).  adv = t + 1 at the first t where any row objects, else
 *    want.
 * 3. Hand-over.  y[b][j], j < adv, goes to out_tokens[b][col + j] and hist[b][pos + 1 + j] (columns outside the arrays skipped),
 *    y[b][adv - 1] to next_token[b * next_stride]; *position += adv, *column += adv, stats += (1, adv); done[b] = fin_b as of
 *    position adv - 1 (an EOS drawn at a position that was not handed over finishes nothing).  adv == 0 moves stats[0] only.
 *    Nothing else is written, except workspace.
 * So the token at output column c of row b is the same function of its prefix's logits and (seed, c, b) as in a decoder that calls
 * eetq_sample_handover_f16 once per column; a position's random number decides something only once every earlier position of
 * the step is confirmed, so using it again after a rollback biases nothing.
 * One workgroup per (b, t), all at once; each publishes its token to workspace and takes a ticket, and the one that arrives last
 * walks and hands over -- nobody waits.  The tickets live in bits 40.. of *position for the length of the launch:
 * -2^39 <= *position < 2^39, nothing else may touch *position meanwhile, and no state is kept between launches.
 * EETQ_ERR_INVALID (nothing launched): every refusal of eetq_spec_accept_f16; a null params or workspace; params or workspace not
 * 8-byte aligned; uniforms given with uniforms_stride < k + 1; batch * (k + 1) >= 2^24. */
int eetq_spec_sample_accept_f16(const void* logits, long stride_b, long stride_t, int vocab, int batch, int k, const int64_t* draft,
                                long draft_stride, int64_t* out_tokens, long out_stride, int out_cols, int64_t* column,
                                int64_t* position, const int64_t* limit, int64_t* next_token, long next_stride, int64_t* hist,
                                long hist_stride, int hist_cols, int64_t* stats, const void* params, int32_t* done,
                                const float* uniforms, long uniforms_stride, int64_t* workspace, void* stream);

/* Single-query (decode) attention over a KV cache; extension used by the EET attention blocks' decode step (the
 * reference delegates the attention product to flash-attn, python/eetq/modules/llama_modules.py:131-143).
 *   out[b][h][:] = softmax_j( scaling * q[b][h] . k[b][h / (heads/kv_heads)][j] + mask[b][j] ) @ v[...]   j < positions
 * fp16 operands, fp32 softmax/accumulation.  strides (in elements): {q_b, q_h, k_b, k_h, k_pos, v_b, v_h, v_pos, mask_b,
 * out_b, out_h}; head_dim (64 or 128) is the dense last dimension everywhere.  mask: additive fp16 [batch][positions]
 * rows (-inf = masked; mask_b may be 0 to share one row) or NULL.  workspace: batch * heads * splits * (head_dim + 4)
 * floats, 16-byte aligned.  A fully masked row gives 0.
 * kv_len (DEVICE int64 scalar or NULL): only cache rows j < min(positions, *kv_len + kv_len_bias) are attended -- the
 * valid length of a pre-allocated cache whose tail holds zeros or stale tokens.  advance (DEVICE int64 scalar or NULL): incremented by one
 * when the call's last kernel finishes (the cache's token counter; may alias kv_len). */
int eetq_decode_attention_f16(const void* q, const void* k_cache, const void* v_cache, const void* mask, void* out,
                              float* workspace, int batch, int heads, int kv_heads, int positions, int head_dim,
                              int splits, float scaling, const long* strides, const int64_t* kv_len, int kv_len_bias,
                              int64_t* advance, void* stream);

/* The chunk count both decode-attention entry points are tuned for (callers size the workspace with it): about two
 * workgroups per compute unit over batch * heads * splits, at most 8, at least 64 cache rows per chunk.  Measured at Llama-13B
 * shapes (tools/attn_bench.py): batch 1 -> 8, batch 2 -> 6, batch 4 -> 3. */
int eetq_decode_attention_splits(int batch, int heads, int positions);

/* Decode step of a pre-allocated KV cache as ONE launch (extension): eetq_rotary_neox_kvcache_f16 followed by
 * eetq_decode_attention_f16, bit-identical to that pair in the cache rows written and in the output.  The new token's q
 * [batch][heads][head_dim] and k [batch][kv_heads][head_dim] are rotated by cos_sin_cache[positions[b]] (rot_dim =
 * head_dim; q is NOT written back), the rotated k and v go to cache row slots[b * slot_stride] (slots NULL: positions[b]),
 * and the rows j < min(max_positions, *kv_len + kv_len_bias) are attended, the new row among them if it is in that range.
 * strides (elements): {q_b, k_b, v_b, kcache_b, kcache_head, kcache_pos, vcache_b, vcache_head, vcache_pos, mask_b,
 * out_b, out_head}.  workspace: batch * heads * splits * (head_dim + 4) floats, 16-byte aligned (contents irrelevant).  tickets: batch *
 * heads + 1 unsigned, ZERO before the first launch that uses them; the launch leaves them zero.  Launches that may run
 * concurrently need distinct workspaces and tickets.  advance: see eetq_decode_attention_f16 (may alias kv_len and slots:
 * it is written after every workgroup of the launch has read them). */
int eetq_rope_decode_attention_f16(const int64_t* positions, const int64_t* slots, int slot_stride, const void* query,
                                   const void* key, const void* value, const void* cos_sin_cache, void* k_cache,
                                   void* v_cache, const void* mask, void* out, float* workspace, unsigned* tickets,
                                   int batch, int heads, int kv_heads, int max_positions, int head_dim, int splits,
                                   float scaling, const long* strides, const int64_t* kv_len, int kv_len_bias,
                                   int64_t* advance, void* stream);
/* ... with the cos|sin table's row count (added within ABI revision 7; table_rows > 0, else EETQ_ERR_INVALID).  The row count is
 * validated but NOT yet enforced on the device: this launch checks no upper bound on positions[b], unlike
 * eetq_rotary_neox_kvcache_bounded_f16 (the compare measured above the run-to-run spread of the decode step's attention term;
 * INTEGRATION.md).  Callers must keep positions[b] < table_rows themselves. */
int eetq_rope_decode_attention_bounded_f16(const int64_t* positions, const int64_t* slots, int slot_stride, const void* query,
                                           const void* key, const void* value, const void* cos_sin_cache, int table_rows,
                                           void* k_cache, void* v_cache, const void* mask, void* out, float* workspace,
                                           unsigned* tickets, int batch, int heads, int kv_heads, int max_positions,
                                           int head_dim, int splits, float scaling, const long* strides, const int64_t* kv_len,
                                           int kv_len_bias, int64_t* advance, void* stream);

/* The decode entries with a PER-ROW FIRST KEY (extension, added within ABI revision 7): eetq_decode_attention_f16 and
 * eetq_rope_decode_attention_bounded_f16 plus kv_start, a DEVICE int64 [batch] array: batch row b of a left-padded batch attends
 * cache rows [s, valid length), s = kv_start[b]; rows below s are padding and are neither read nor written.  The K, V and mask bases
 * move by s rows and the valid length and the slot are taken relative to s, so blocks and chunks are counted from the row's first
 * real token: out[b] has the bits of the twin entry called on row b alone, on a cache of the same capacity whose rows [0, S - s)
 * are this cache's rows [s, S), with slots - s and kv_len - s and the same splits, mask (moved by s) and scaling.  The new token
 * is written at its absolute slot; advance, tickets, workspace and the dropped-step counter as in the twins; the two forms stay
 * bit-identical to each other.  s is kept inside [0, slot] (one-launch form) or [0, valid length - 1] (two-launch form): a start
 * beyond it is a caller error that attends that one row and touches nothing outside the cache.  All-zero kv_start: the twin's bits.
 * Errors as the twins, plus a null kv_start (EETQ_ERR_INVALID, nothing launched). */
int eetq_decode_attention_padded_f16(const void* q, const void* k_cache, const void* v_cache, const void* mask, void* out,
                                     float* workspace, int batch, int heads, int kv_heads, int positions, int head_dim,
                                     int splits, float scaling, const long* strides, const int64_t* kv_len, int kv_len_bias,
                                     const int64_t* kv_start, int64_t* advance, void* stream);
int eetq_rope_decode_attention_padded_f16(const int64_t* positions, const int64_t* slots, int slot_stride, const void* query,
                                          const void* key, const void* value, const void* cos_sin_cache, int table_rows,
                                          void* k_cache, void* v_cache, const void* mask, void* out, float* workspace,
                                          unsigned* tickets, int batch, int heads, int kv_heads, int max_positions,
                                          int head_dim, int splits, float scaling, const long* strides, const int64_t* kv_len,
                                          int kv_len_bias, const int64_t* kv_start, int64_t* advance, void* stream);

/* The decode entries with a SLIDING WINDOW (extension, added within ABI revision 7): the padded entries plus `window` >= 1, a host
 * integer (a constant of the model: one captured graph serves a decoder).  Batch row b attends the last `window` of its n valid
 * rows, and never a row below kv_start[b]: out[b], the cache rows written and every side effect are those of the padded entry
 * called with kv_start'[b] = max(kv_start[b], n - window), bit for bit, and rows below kv_start' are neither read nor written.
 * n is the valid length the kernel derives: in the one-launch form slot + 1 (the new token counts; without a new token -- a slot
 * outside the cache -- clamp(*kv_len + kv_len_bias), or max_positions without kv_len), in the two-launch form clamp(*kv_len +
 * kv_len_bias) or `positions`.  kv_start may be NULL (all zeros).  window >= n: the padded entry's bits with kv_start as given.  The
 * two forms stay bit-identical to each other; no launch is added.  Errors as the padded entries (a null kv_start is none), plus
 * window < 1 (EETQ_ERR_INVALID, nothing launched).  fp16 rows only: the int8 entries have no windowed form. */
int eetq_decode_attention_window_f16(const void* q, const void* k_cache, const void* v_cache, const void* mask, void* out,
                                     float* workspace, int batch, int heads, int kv_heads, int positions, int head_dim,
                                     int splits, float scaling, const long* strides, const int64_t* kv_len, int kv_len_bias,
                                     const int64_t* kv_start, int window, int64_t* advance, void* stream);
int eetq_rope_decode_attention_window_f16(const int64_t* positions, const int64_t* slots, int slot_stride, const void* query,
                                          const void* key, const void* value, const void* cos_sin_cache, int table_rows,
                                          void* k_cache, void* v_cache, const void* mask, void* out, float* workspace,
                                          unsigned* tickets, int batch, int heads, int kv_heads, int max_positions,
                                          int head_dim, int splits, float scaling, const long* strides, const int64_t* kv_len,
                                          int kv_len_bias, const int64_t* kv_start, int window, int64_t* advance, void* stream);

/* THE RING CACHE (extension, added within ABI revision 7): the capacity half of the sliding window.  k_cache / v_cache hold R =
 * `ring_rows` rows and logical cache row r -- the token's position in the sequence, from 0, unbounded -- lives at physical row
 * r mod R.  Keys are stored rotated, so a row carries its position and nothing is re-rotated.  Everything the windowed entries
 * compute stays in logical rows (the valid length n, the first attended row max(0, n - window), blocks, chunks, shares, masks);
 * only the address of a row changes.  The contract: each ring entry returns THE BITS of its windowed entry (same window, same
 * splits, same LONG form -- decided by the capacity passed: R here) called on a static cache that holds the same logical rows, and
 * the one-launch entry writes the new row at physical row slot mod R and no other.  kv_len is REQUIRED and counts logical rows (it
 * may exceed R); `slots` / positions are logical as well: a ring is never full, so only a negative slot or position drops a step.
 * Decode entries: R >= window (EETQ_ERR_INVALID below; the live rows of a step are n - window .. n - 1).  No kv_start and no mask
 * (their arguments are gone).  Default splits as the static entries, taken from R -- untuned for rings.
 * Every row of the ring must hold finite values (allocate zeros; stale rows are old real rows): see the prompt entry. */
int eetq_decode_attention_ring_f16(const void* q, const void* k_cache, const void* v_cache, void* out, float* workspace, int batch,
                                   int heads, int kv_heads, int ring_rows, int head_dim, int splits, float scaling,
                                   const long* strides, const int64_t* kv_len, int kv_len_bias, int window, int64_t* advance,
                                   void* stream);
int eetq_rope_decode_attention_ring_f16(const int64_t* positions, const int64_t* slots, int slot_stride, const void* query,
                                        const void* key, const void* value, const void* cos_sin_cache, int table_rows,
                                        void* k_cache, void* v_cache, void* out, float* workspace, unsigned* tickets, int batch,
                                        int heads, int kv_heads, int ring_rows, int head_dim, int splits, float scaling,
                                        const long* strides, const int64_t* kv_len, int kv_len_bias, int window, int64_t* advance,
                                        void* stream);

/* The int8 KV cache (extension, added within ABI revision 7).  One cache ROW is the head_dim fp16 values of one (batch row, kv
 * head, position); rows are quantised symmetrically, each with a scale of its own:
 *   amax = max_d |x_d| (exact);  s = fp16(fp32(amax) * (1.0f / 127.0f)), one fp32 multiply, round to nearest even;
 *   q_d = clamp(round_half_away(fp32(x_d) / fp32(s)), -127, 127) as int8, IEEE fp32 division (eetq_quant_weights' rounding);
 *   -128 is never written, s == 0 gives q = 0, non-finite inputs are outside the contract.
 * Storage: k_cache_i8 and v_cache_i8 are int8 [batch][kv_heads][positions][head_dim], plain two's complement; kv_scales is fp16
 * [batch][kv_heads][positions][2] = (k scale, v scale) of the row, one dword per row.  Attention is over the dequantised rows
 * ks * k8 and vs * v8 taken as exact reals, with fp32 scores, softmax state and accumulation as in the fp16 entries: the K scale is
 * folded into the score, (ks * scaling) * (q . k8), the V scale into the probability, (p * vs) * v8.  vs * v8 is exact in fp32, so a
 * row that holds all the weight comes out as fp16(vs * v8) bit for bit.
 *
 * eetq_decode_attention_i8kv_f16: eetq_decode_attention_f16 over such a cache.  strides: as there, with the k / v entries in BYTES
 * ({q_b, q_h, k_b, k_h, k_pos, v_b, v_h, v_pos, mask_b, out_b, out_h}); scale_strides (fp16 elements): {batch, head, position}.
 * Workspace, splits (eetq_decode_attention_splits), mask, kv_len, kv_len_bias and advance as in the fp16 entry.
 * EETQ_ERR_INVALID (nothing launched): a null pointer; a cache stride that is not a multiple of 8 bytes or a cache that is not
 * 8-byte aligned (8-byte loads); a scale stride that is not a multiple of 2 elements or scales that are not 4-byte aligned; a q
 * stride that is not a multiple of 8 elements or a q that is not 16-byte aligned; (positions + 4096) * the row stride in bytes (of
 * a cache or of the scales) >= 2 GiB.  EETQ_ERR_UNSUPPORTED: head_dim other than 64 or 128. */
int eetq_decode_attention_i8kv_f16(const void* q, const void* k_cache_i8, const void* v_cache_i8, const void* kv_scales,
                                   const void* mask, void* out, float* workspace, int batch, int heads, int kv_heads, int positions,
                                   int head_dim, int splits, float scaling, const long* strides, const long* scale_strides,
                                   const int64_t* kv_len, int kv_len_bias, int64_t* advance, void* stream);

/* eetq_rope_decode_attention_bounded_f16 on an int8 cache, ONE launch: K is quantised after the rotation (the rotation's bits are
 * those of the fp16 entries), the row's bytes and scale pair are written from registers to row slots[b * slot_stride], and the new
 * token enters the softmax as its quantised self -- the same (k8, ks, v8, vs) -- from registers: nothing in the launch reads what
 * the launch writes, and the result equals "write the row, then eetq_decode_attention_i8kv_f16" bit for bit.  strides: as the fp16
 * entry, cache entries in bytes; scale_strides as above; tickets, workspace, advance as the fp16 entry; table_rows is validated
 * and not enforced on the device, as there.  A slot outside the cache (or a negative position) is neither written nor attended,
 * and counted (eetq_decode_dropped_steps).  Errors as eetq_decode_attention_i8kv_f16, plus q / k / v strides that are not
 * multiples of 8 elements, a q, k, v or cos|sin table that is not 16-byte aligned, table_rows <= 0, slot_stride not 0 or 1. */
int eetq_rope_decode_attention_i8kv_f16(const int64_t* positions, const int64_t* slots, int slot_stride, const void* query,
                                        const void* key, const void* value, const void* cos_sin_cache, int table_rows,
                                        void* k_cache_i8, void* v_cache_i8, void* kv_scales, const void* mask, void* out,
                                        float* workspace, unsigned* tickets, int batch, int heads, int kv_heads, int max_positions,
                                        int head_dim, int splits, float scaling, const long* strides, const long* scale_strides,
                                        const int64_t* kv_len, int kv_len_bias, int64_t* advance, void* stream);

/* eetq_rotary_neox_kvcache_prefill_bounded_f16 writing an int8 cache: query [batch][tokens][q_heads][head_size] AND key are rotated
 * IN PLACE (key is writable: a prompt then attends the rotated fp16 K where it lies, unquantised), and the rotated key and the
 * value of every (token, kv head) are quantised by the rule above and written to rows base + t of the caches and of kv_scales, base
 * = *first_row_dev (DEVICE int64, read and not advanced) or first_row.  tokens = 1 with first_row_dev = the cache's counter is the
 * cache write of an unfused decode step.  strides: {q_token, k_token, v_token (elements), cache_b, cache_head, cache_row (bytes,
 * shared by both caches)}; scale_strides as above.  Tokens whose row lies outside [0, max_positions) or whose position lies outside
 * [0, table_rows) are left untouched and counted (eetq_decode_dropped_steps).  EETQ_ERR_INVALID: null pointers, token strides that
 * are not multiples of 8 elements, q / k / v / table not 16-byte aligned, cache strides not multiples of 8 bytes or caches not 8-byte
 * aligned, scale strides not multiples of 2 or scales not 4-byte aligned, rot_dim != head_size, rows outside the cache (host
 * first_row), table_rows <= 0.  EETQ_ERR_UNSUPPORTED: head_size other than 64 or 128. */
int eetq_rotary_neox_kvcache_prefill_i8_f16(const int64_t* positions, void* query, void* key, const void* value,
                                            const void* cos_sin_cache, int table_rows, void* k_cache_i8, void* v_cache_i8,
                                            void* kv_scales, int batch, int tokens, const int64_t* first_row_dev, int first_row,
                                            int q_heads, int k_heads, int head_size, int rot_dim, const long* strides,
                                            const long* scale_strides, int max_positions, void* stream);

/* Causal attention over a PROMPT on the matrix cores (extension, ABI revision 6): out[b][t][h] = softmax_j<=t+causal_offset(scaling
 * q[b][t][h] . k[b][h / groups][j]) v[b][h / groups][j] over the first `keys` rows of a KV cache, fp16 in / out, fp32 scores, softmax
 * state and accumulation (probabilities rounded to fp16 for the second product, like flash-attn, which the reference's block calls
 * here: python/eetq/modules/llama_modules.py:131-143).  q: the rotated query rows, e.g. a view into the fused QKV projection's
 * output; k, v: cache tensors [batch][kv_heads][rows][head_dim].  strides (elements): {q_b, q_token, q_head, k_b, k_head, k_row,
 * v_b, v_head, v_row, out_b, out_token, out_head}, head_dim contiguous, q / k / v strides multiples of 8, out strides of 4.
 * causal_offset = keys - q_tokens for a prompt appended to `keys - q_tokens` cached rows (0 on an empty cache).  head_dim 64 or 128
 * (eetq_prefill_attention_supported); EETQ_ERR_UNSUPPORTED otherwise. */
int eetq_prefill_attention_f16(const void* q, const void* k, const void* v, void* out, int batch, int heads, int kv_heads, int q_tokens,
                               int keys, int head_dim, int causal_offset, float scaling, const long* strides, void* stream);
int eetq_prefill_attention_supported(int head_dim);

/* ... with the number of keys read on the DEVICE, and optionally split over the keys (added within ABI revision 7).  Every workgroup
 * reads *kv_len (DEVICE int64 scalar) at entry and attends keys = clamp(*kv_len + kv_len_bias, 0, max_keys) cache rows with
 * causal_offset = keys - q_tokens: a prompt appended behind the rows a static cache already holds, its counter already advanced.  Per
 * query row the arithmetic is that of eetq_prefill_attention_f16 with the same keys, bit for bit; keys <= 0 gives zeros.  Nothing is read
 * on the host: the call can be captured.  kv_len NULL: keys = max_keys (the split form with a host length).  strides as above; the
 * 2 GiB range rule is checked against max_keys.
 * splits == 1: one launch, workspace may be NULL.  splits in 2 .. eetq_prefill_attention_max_splits() (16): each (query block, head,
 * batch row) becomes `splits` workgroups, share i taking the key blocks [i n / splits, (i + 1) n / splits) of that workgroup's n
 * blocks of 64 keys; every share leaves its unnormalised fp32 accumulators and (maximum, sum) per query row in `workspace` -- an
 * empty share (-inf, 0, zeros), so the workspace's previous contents never matter -- and a second launch merges them (weights
 * exp2(m_i - max m), one division).  No atomics, no tickets; deterministic.  workspace: DEVICE,
 * eetq_prefill_attention_workspace_floats(batch, heads, q_tokens, head_dim, splits) = batch * heads * q_tokens * splits *
 * (head_dim + 2) floats, 16-byte aligned; launches that may run concurrently need distinct workspaces.
 * EETQ_ERR_INVALID: null q / k / v / out / strides, max_keys <= 0, splits < 1 or > 16, splits > 1 with a NULL or misaligned
 * workspace, the stride and alignment rules above; EETQ_ERR_UNSUPPORTED: head_dim. */
int eetq_prefill_attention_dev_f16(const void* q, const void* k, const void* v, void* out, float* workspace, int batch, int heads,
                                   int kv_heads, int q_tokens, int max_keys, int head_dim, const int64_t* kv_len, int kv_len_bias,
                                   int splits, float scaling, const long* strides, void* stream);
/* eetq_prefill_attention_dev_f16 with a PER-ROW FIRST KEY (added within ABI revision 7): kv_start is a DEVICE int64 [batch] array,
 * kv_start[b] the first real cache row of batch row b of a left-padded batch.  With keys as above, koff = keys - q_tokens (query t
 * sits at cache row koff + t) and p = clamp(kv_start[b] - koff, 0, q_tokens) pad queries: out[b][:p] is ZEROS; out[b][p:] has the
 * bits of eetq_prefill_attention_dev_f16 called on row b alone with q, k, v and out moved to the first real row -- q_tokens - p
 * queries, keys - kv_start[b] keys, the same splits and scaling -- i.e. key blocks, query blocks and split shares are counted from
 * the row's first real token; no cache row below kv_start[b] is read.  All-zero kv_start: the bits of the plain entry.  kv_len NULL:
 * keys = max_keys (a fresh prompt).  Workspace and splits as there.  Errors as there, plus a null kv_start. */
int eetq_prefill_attention_padded_f16(const void* q, const void* k, const void* v, void* out, float* workspace, int batch, int heads,
                                      int kv_heads, int q_tokens, int max_keys, int head_dim, const int64_t* kv_len, int kv_len_bias,
                                      const int64_t* kv_start, int splits, float scaling, const long* strides, void* stream);
/* eetq_prefill_attention_dev_f16 with a SLIDING WINDOW (added within ABI revision 7): `window` >= 1 is a host integer.  With keys and
 * koff = keys - q_tokens as above, query t sits at cache row p = t + koff and attends rows max(0, p - window + 1) .. p: itself and the
 * window - 1 rows before it.  The key blocks stay blocks of 64 from row 0; a workgroup with first query q0 runs blocks
 * [jlo, n), jlo = max(0, q0 + koff - window + 1) / 64, and with splits > 1 share i takes [jlo + i m / splits, jlo + (i + 1) m / splits)
 * of its m = n - jlo blocks.  Two consequences: (a) window >= keys gives the bits of eetq_prefill_attention_dev_f16 for every row, and
 * in any launch every row with t + koff < window has that entry's bits; (b) no cache row below 64 * (max(0, koff - window + 1) / 64) is
 * read by the launch -- rows of a lower-edge block below a row's window ARE read and enter the value product with probability 0, so
 * they must be finite (they are the sequence's own tokens).  kv_len NULL: keys = max_keys (a fresh prompt).  Workspace and splits as
 * there; callers that follow the library's rule size the shares with eetq_prefill_attention_splits(batch, heads, q_tokens,
 * min(max_keys, window + min(q_tokens, 128))), an UNTUNED rule.  Errors as there, plus window < 1.  fp16 rows, one shared first key:
 * there is no windowed form of the per-row first key or of the int8-row entry. */
int eetq_prefill_attention_window_f16(const void* q, const void* k, const void* v, void* out, float* workspace, int batch, int heads,
                                      int kv_heads, int q_tokens, int max_keys, int head_dim, const int64_t* kv_len, int kv_len_bias,
                                      int window, int splits, float scaling, const long* strides, void* stream);
/* eetq_prefill_attention_window_f16 on a RING cache ("The ring cache" above): k / v hold `ring_rows` rows, max_keys and kv_len count
 * logical rows (max_keys <= 2^30, it may exceed ring_rows), and key block j is read from physical block j mod (ring_rows / 64).
 * The bits of the windowed entry on a static cache of the same logical rows.  ring_rows % 64 == 0 (a key block never straddles the
 * ring's end) and ring_rows >= window + q_tokens + 62 (EETQ_ERR_INVALID otherwise): the lowest row a launch reads is
 * 64 floor((koff - window + 1) / 64) >= koff - window - 62, the highest row the call's cache write has just replaced, koff +
 * q_tokens - 1, aliases logical row koff + q_tokens - 1 - ring_rows, and the rule keeps the second below the first.  Rows of the
 * upper-edge block at and beyond the keys -- clipped by the descriptor on a static cache -- are rows of the ring here, stale or
 * never written; like the rows of a lower-edge block below a window they are read and enter the value product with probability
 * 0, so EVERY row of the ring must be finite.  Splits and workspace as the windowed entry (same untuned rule). */
int eetq_prefill_attention_ring_f16(const void* q, const void* k, const void* v, void* out, float* workspace, int batch, int heads,
                                    int kv_heads, int q_tokens, int max_keys, int head_dim, const int64_t* kv_len, int kv_len_bias,
                                    int window, int ring_rows, int splits, float scaling, const long* strides, void* stream);
/* The split count eetq_prefill_attention_dev_f16 is tuned for (pure host function; callers size the workspace with it; 1 = unsplit).
 * With g = ceil(q_tokens / 128) * heads * batch workgroups and n = ceil(max_keys / 64) key blocks: the largest power of two s <= 16
 * such that, for every power of two s' <= s, s' g <= 1.25 compute units and n / s' >= 4 (s' g <= half the compute units), 8 (s' g <=
 * all of them) or 16 (beyond).  1 wherever g alone fills the chip.  Measured at 40 x 128 and 32 / 8 x 128 heads
 * (tools/prefill_attn_bench.py --append, profiles/prefill_attn_append.txt): more than 1 only where the split form beat the unsplit
 * host-length call. */
int    eetq_prefill_attention_splits(int batch, int heads, int q_tokens, int max_keys);
int    eetq_prefill_attention_max_splits(void);
size_t eetq_prefill_attention_workspace_floats(int batch, int heads, int q_tokens, int head_dim, int splits);

/* FEW-ROW attention behind a long cache (added within ABI revision 7): `rows` = 1 .. 16 query rows per batch row -- the last `rows`
 * rows a static fp16 KV cache has just been given, rotated (a speculative verify step, a chunked prompt's short last piece) -- attend
 * the cache causally among themselves, split over the keys, both products on the 16x16x32 matrix-core shape.  Semantics are exactly
 * those of eetq_prefill_attention_dev_f16:
 *   keys = clamp(*kv_len + kv_len_bias, 0, max_keys); kv_len NULL means keys = max_keys;
 *   koff = keys - rows;
 *   query t attends cache rows j with 0 <= j <= min(keys - 1, koff + t);
 *   out[b][t][h] = softmax_j(scaling * q[b][t][h] . k[b][h / groups][j]) . v[b][h / groups][j];
 *   a query with nothing to attend gives zeros (koff + t < 0, and keys = 0);
 *   rows at or beyond keys are never read (they hold stale drafts or NaN).
 * fp16 in and out; scores, softmax state and accumulators fp32; the probabilities enter the second product as fp16, carried as 2^12 p.
 * q: the strided [batch][rows][heads][head_dim] view into the fused QKV output; caches [batch][kv_heads][rows][head_dim] with any
 * batch / head / row strides, head_dim contiguous.  strides: the twelve of eetq_prefill_attention_f16 in the same order ({q_b, q_row,
 * q_head, k_b, k_head, k_row, v_b, v_head, v_row, out_b, out_row, out_head}, elements), q / k / v strides multiples of 8, out strides
 * of 4, q / k / v 16-byte aligned, out 8-byte.  head_dim 64 or 128, any heads % kv_heads == 0: the heads / kv_heads * rows (head, query
 * row) pairs of a kv head are one tile, a K / V row is loaded once per kv head.
 * CHUNK RULE: with n = ceil(keys / 32) blocks of 32 key rows, chunk i of `splits` owns blocks [floor(i n / splits),
 * floor((i + 1) n / splits)), i.e. key rows [32 floor(i n / splits), min(keys, 32 floor((i + 1) n / splits))); a chunk may be empty.
 * Always two launches: one workgroup per (chunk, kv head, batch row) leaves, per (query row, head), the record [m, l, -, -,
 * o[head_dim]] in `workspace` -- an empty chunk or a row with nothing to attend in it (-inf, 0, zeros), so the workspace's previous
 * contents never matter -- and a second launch merges a row's records (weights exp2(m_i - max m), one division; a fully masked row
 * gives zeros).  No atomics, no tickets, no state between launches; deterministic.  Nothing is read on the host: capturable.
 * workspace: DEVICE, eetq_decode_attention_rows_workspace_floats(batch, heads, rows, head_dim, splits) = batch * heads * rows *
 * splits * (head_dim + 4) floats, 16-byte aligned, needed at every `splits` (also 1); launches that may run concurrently need
 * distinct workspaces.
 * EETQ_ERR_INVALID (nothing launched): null q / k_cache / v_cache / out / strides, rows outside 1 .. 16, max_keys <= 0, splits outside
 * 1 .. eetq_decode_attention_rows_max_splits() (64), a NULL or misaligned workspace, the stride and alignment rules above, one head's
 * cache rows spanning 2 GiB or more (checked against max_keys).  EETQ_ERR_UNSUPPORTED: head_dim other than 64 or 128. */
int    eetq_decode_attention_rows_f16(const void* q, const void* k_cache, const void* v_cache, void* out, float* workspace, int batch,
                                      int heads, int kv_heads, int rows, int max_keys, int head_dim, const int64_t* kv_len,
                                      int kv_len_bias, int splits, float scaling, const long* strides, void* stream);
/* The chunk count the entry is tuned for (pure host function; callers size the workspace with it): with g = batch * kv_heads *
 * ceil(heads / kv_heads * rows / 64) workgroups per chunk, n = ceil(max_keys / 32) blocks and r = 2 workgroups per compute unit
 * where heads / kv_heads * rows <= 16 (one sub-tile), else 1: min(r * compute units / g, max(n / 8, min(8, n / 4)), 32), at least 1
 * (integer divisions) -- the grid fills the chip once, a chunk keeps 4 blocks up to 8 chunks and 8 beyond, never more than 32
 * chunks.  Tuned from tools/attn_rows_bench.py's table (profiles/attn_rows.txt). */
int    eetq_decode_attention_rows_splits(int batch, int heads, int kv_heads, int rows, int max_keys);
int    eetq_decode_attention_rows_max_splits(void);
size_t eetq_decode_attention_rows_workspace_floats(int batch, int heads, int rows, int head_dim, int splits);

/* eetq_prefill_attention_dev_f16 over an int8 KV cache (the row format above; added within ABI revision 7): a prompt appended behind
 * int8 rows, its own rows already written (rotated, quantised) and the counter advanced, attends the dequantised rows 0 .. keys - 1,
 * causally among its own -- a query token sees its own key and value as their quantised selves, as the one-launch decode step does.
 * kv_len, kv_len_bias, splits and workspace (eetq_prefill_attention_workspace_floats, eetq_prefill_attention_splits) as in
 * eetq_prefill_attention_dev_f16; kv_len NULL: keys = max_keys.  Rows at and beyond keys are not read.  strides: as the fp16 entry,
 * with the k / v entries in BYTES; scale_strides (fp16 elements): {batch, head, position}.
 * Arithmetic: the tiles, the fp32 softmax state, the fp16 probabilities and the split records of the fp16 entry.  K bytes enter the
 * first product as exact fp16 integers and the K scale is folded into the fp32 score behind it, (ks * scaling) * (q . k8), as in the
 * decode entries.  ONE DIFFERENCE from the decode entries: a V row enters the second product as fp16(vs * v8) -- one rounding of the
 * exact product, denormals kept -- instead of vs riding on the probability in fp32 (the probabilities here are fp16 operands carried
 * as 2^12 p, and 2^12 p * vs would leave the fp16 range).  A row that holds all the weight still comes out as fp16(vs * v8) bit
 * for bit.
 * EETQ_ERR_INVALID (nothing launched): the cache, scale and 2 GiB rules of eetq_decode_attention_i8kv_f16 (against max_keys), the q
 * and out rules of eetq_prefill_attention_f16, a null pointer, max_keys <= 0, splits < 1 or > 16, splits > 1 with a NULL or
 * misaligned workspace.  EETQ_ERR_UNSUPPORTED: head_dim other than 64 or 128. */
int eetq_prefill_attention_i8kv_f16(const void* q, const void* k_cache_i8, const void* v_cache_i8, const void* kv_scales, void* out,
                                    float* workspace, int batch, int heads, int kv_heads, int q_tokens, int max_keys, int head_dim,
                                    const int64_t* kv_len, int kv_len_bias, int splits, float scaling, const long* strides,
                                    const long* scale_strides, void* stream);

/* eetq_decode_attention_rows_f16 over an int8 KV cache (the row format above; added within ABI revision 7): `rows` = 1 .. 16 query rows
 * per batch row, their own cache rows already written (rotated, quantised) and the counter advanced, attend the DEQUANTISED rows
 * 0 .. keys - 1 causally among themselves -- a speculative verify step on an int8 cache.  Semantics, kv_len, kv_len_bias, the CHUNK
 * RULE, the two launches, the records and the workspace are eetq_decode_attention_rows_f16's: koff = keys - rows, query t attends rows
 * 0 .. min(keys - 1, koff + t), rows at and beyond keys are never read (bytes and scales there may be anything, NaN scales included), a
 * query with nothing to attend gives zeros.  eetq_decode_attention_rows_splits, _max_splits and _workspace_floats serve both entries
 * (the chunk rule was tuned on fp16 rows and is reused as it is).  strides: as the fp16 entry, with the k / v entries in BYTES;
 * scale_strides (fp16 elements): {batch, head, position}.
 * Arithmetic: that of eetq_prefill_attention_i8kv_f16 on this kernel's tiles.  K bytes enter the first product as exact fp16 integers
 * and the K scale is folded into the fp32 score behind it, per key, before the mask: (ks * scaling * log2 e) * (q . k8), the softmax in
 * base 2.  As in the prompt entry, and UNLIKE the decode entries (which fold vs into the probability in fp32), a V row enters the second
 * product as fp16(vs * v8) -- one rounding of the exact product, denormals kept: the probabilities are fp16 operands carried as 2^12 p,
 * and 2^12 p * vs would leave the fp16 range.  A row that holds all the weight comes out as fp16(vs * v8) bit for bit.
 * EETQ_ERR_INVALID (nothing launched): the cache, scale and 2 GiB rules of eetq_decode_attention_i8kv_f16 (against max_keys), a cache
 * row stride below head_dim bytes, the q / out / rows / splits / workspace rules of eetq_decode_attention_rows_f16, a null pointer,
 * max_keys <= 0.  EETQ_ERR_UNSUPPORTED: head_dim other than 64 or 128. */
int eetq_decode_attention_rows_i8kv_f16(const void* q, const void* k_cache_i8, const void* v_cache_i8, const void* kv_scales, void* out,
                                        float* workspace, int batch, int heads, int kv_heads, int rows, int max_keys, int head_dim,
                                        const int64_t* kv_len, int kv_len_bias, int splits, float scaling, const long* strides,
                                        const long* scale_strides, void* stream);

/* Diagnostics: while `stamps` (DEVICE, batch * heads * splits * 8 uint64) is set, every eetq_rope_decode_attention_f16
 * launch of this process records per workgroup the 100 MHz device clock at: 0 entry, 1 scalar reads done, 2 new token
 * rotated, 3 chunk done, 4 chunk record published, 5 ticket drawn, 6 (last workgroup of a head) merge done, 7 output
 * stored.  NULL switches it off.  Used by tools/attn_bench.py --stamps; not for production launches. */
int eetq_diag_attn_stamps(unsigned long long* stamps);

/* ---- profiling hook (no reference counterpart; used by bench.py) -------------------------------------
 * Between eetq_prof_begin(n) and eetq_prof_end() every kernel this library launches from the calling thread
 * carries a start/stop event pair on its dispatch packet; eetq_prof_end synchronises the device and returns
 * the kernel durations in microseconds, in launch order (*count = launches recorded, <= n).  Not capturable
 * into a HIP graph. */
int eetq_prof_begin(int max_launches);
int eetq_prof_end(float* durations_us, int capacity, int* count);
/* Diagnostic: a kernel that only reads `bytes` (multiple of 64 KiB) from p with the GEMV's load pattern; its
 * duration is the read floor for that many bytes on this chip.  `sink` = 4 writable device bytes. */
int eetq_diag_stream_read(const void* p, size_t bytes, void* sink, void* stream);
/* Diagnostic: a kernel of `grid` x `block` threads that touches no memory (the fixed cost of a dispatch, and the resolution
 * floor of the timing method it is measured with). */
int eetq_diag_empty(void* sink, int grid, int block, void* stream);
/* Diagnostic: `grid` one-wave workgroups each record {XCC_ID, HW_ID, s_memtime (shader cycles), s_memrealtime (100 MHz)} into
 * out[4 * workgroup .. +3] (DEVICE, grid * 4 uint64).  Two launches around a chain of kernels give the average shader clock
 * the chip held over the chain, per XCD: d(memtime) / d(memrealtime) x 100 MHz (bench.py `effective_clock_mhz`: the
 * evidence for "power-bound").  Graph-capturable. */
int eetq_diag_clock_stamp(unsigned long long* out, int grid, void* stream);
/* Diagnostic, host arithmetic only (no launch; with cus > 0 no device either): which plan the small-batch kernel (1 <= M <= 16 rows;
 * AUTO sends 2 <= M <= 16 there, except narrow deep W8A16 weights from M = 9: eetq_diag_auto_path) takes for a weight of `bits` (8 / 4), K x N, on a chip with `cus` compute units (<= 0: the current
 * device's).  *form = 0 activation fragments straight from L2 into registers, 1 rows copied once per workgroup into LDS, 2 per-wave
 * LDS-DMA ring; *tile_rows = 16-column tile rows per workgroup (1 / 2); *waves = waves per workgroup.  All plans give the same bits
 * at equal *waves.  The environment overrides (EETQ_AMD_I8_STREAM_PLAN ...) are not applied.  No reference counterpart: the
 * reference picks its CUTLASS tile by a timing sweep at run time (cutlass_heuristic.cc), this library by a rule -- this entry shows it. */
int eetq_diag_stream_plan(int bits, int M, int N, int K, int cus, int* form, int* tile_rows, int* waves);
/* Diagnostic, host arithmetic only (no launch): which kernel path EETQ_PATH_AUTO takes for an M x K activation against a K x N
 * weight of `bits` (8 / 4) on the current device.  *path = EETQ_PATH_* (for bits = 4: GEMV, STREAM, SPLITK, or MFMA = expansion to
 * int8 tiles + the W8A16 kernels); *detail (may be NULL) = K slices per tile when *path is EETQ_PATH_TILESPLIT (1 = the unsplit
 * tiled kernel), the row groups of the plan when *path is EETQ_PATH_SPLITK (0 = K slices only), else 0.  It calls the function the launchers call.  Replaces, as far as anything does, the reference's run-time
 * choice: the m <= 4 switch (fpA_intB_gemm_wrapper.cu:149-162) and the occupancy-scored tile pick
 * (cutlass_kernels/cutlass_heuristic.cc:123-206) -- one rule here, printed by bench.py's `config4` block per point and measured
 * against every forced path by tools/auto_regret.py. */
int eetq_diag_auto_path(int bits, int M, int N, int K, int* path, int* detail);

/* Diagnostic, host arithmetic only: the plan the split-K medium-batch tile (EETQ_PATH_SPLITK, W8A16 and W4A16 alike) runs an M x K
 * activation against a K x N weight with -- *column_blocks (32-column blocks per workgroup: 1 or 2), *k_slices (1, 2 or 4; > 1
 * needs the stream's scratch region), *ring (10 * activation stages + weight stages: 22 or 33), *row_groups (the batch cut along
 * M; M <= 32 * 4 * row_groups).  It calls the planner the launcher calls (gemm_splitk.hip::splitk_plan: one cost model over every
 * combination, its constants fitted on the measured time of every plan -- profiles/r05_splitk_plan_regret*.jsonl), so
 * tests/test_abi.py can hold the planner against those tables without a GPU.  1 <= M <= 1024, K % 64 == 0. */
int eetq_diag_splitk_plan(int M, int N, int K, int* column_blocks, int* k_slices, int* ring, int* row_groups);

/* Diagnostic, host arithmetic only (no launch; with cus > 0 no device either; added within ABI revision 7): the launches the
 * LDS-tiled MFMA kernel's dense launchers make for an M x K activation against a K x N weight of `bits` -- 8: eetq_w8a16_gemm_ex
 * (EETQ_PATH_MFMA) with epilogue `act` (EETQ_ACT_*), tile_j = 0; 4: eetq_w4a16_gemm_tiled with its tile_j (0 = the rule, 1 =
 * 128 x 64, 2 = 128 x 128), act = 0 -- on a chip with `cus` compute units (<= 0: the current device's).  One record of six ints per
 * launch, in launch order: {row0, rows, col0, cols, tile, k_slices}; tile = 2 the 128 x 128 tile, 1 the 128 x 64 tile, 0 a 64-row
 * chunk of the small-batch kernel (bits = 8, K < 320).  *count = the number of launches; the first min(*count, max_records)
 * records are written.  It walks the planner the launchers walk (csrc/gemm_tile_plan.hpp) and reports what that planner ASKS for:
 * k_slices = 2 (the ragged last round of wide tiles in two K slices of the narrow tile) needs the stream's split-K scratch region,
 * and a launch runs that segment unsplit, with the tile shape the record names, when the stream has none or EETQ_AMD_SPLITK=0.
 * EETQ_ERR_UNSUPPORTED for what the launcher of these bits refuses (bits = 4: K % 128 != 0, K < 384, act != 0; either: an operand
 * beyond the 32-bit buffer offsets); EETQ_ERR_INVALID for a null pointer or other bits. */
int eetq_diag_tile_plan(int bits, int M, int N, int K, int act, int tile_j, int cus, int* records, int max_records, int* count);

/* Decode steps on a pre-allocated KV cache (eetq_rope_decode_attention_f16, eetq_rotary_neox_kvcache_f16) whose new token
 * was NOT written because its cache row lies outside the cache (slot >= rows: the cache is full; or a negative position) or,
 * through the *_bounded entries, because its position lies outside the cos|sin table; tokens that the plain rotary entries
 * left unrotated for that reason are counted here too.
 * The kernels skip the write instead of faulting (stock transformers raises an index error there); this entry synchronises
 * the current device and reports how many such steps its kernels have dropped since the last reset (batch rows count
 * individually), optionally resetting the count.  A non-zero count means the tokens generated after that point are wrong. */
int eetq_decode_dropped_steps(unsigned long long* count, int reset);

/* ---- library-owned scratch ---------------------------------------------------------------------------
 * The reference's operators take no workspace argument (fpA_intB_gemm_wrapper.cu:169-170 passes none), so the few
 * buffers the kernels need are owned by the library: the split-K partial-tile regions (40 MiB per launch stream that
 * ever ran a 17 <= M <= 128 GEMM, at most EETQ_AMD_SPLITK_REGIONS (default 16) per device; a stream that cannot get a
 * region of its own runs unsplit -- regions are never shared), the W4A16 prefill expansion buffers and the quantiser's
 * NULL-workspace buffer.  eetq_release_workspace synchronises the devices that hold any, frees all of it and reports the
 * bytes freed (bytes_freed may be NULL); later calls re-create what they need.  Do not call it while a HIP graph that
 * captured a split-K or W4A16 launch is still going to be replayed. */
int eetq_release_workspace(size_t* bytes_freed);
/* Gives the split-K region owned by `stream` (current device) back to the pool after synchronising the stream; call it
 * before destroying a stream that ran 17 <= M <= 128 GEMMs, unless HIP graphs captured on it are still going to be
 * replayed.  The library never reclaims a region on its own: once all regions are owned, further streams run the unsplit
 * kernels.  EETQ_OK also when the stream owns nothing. */
int eetq_release_stream_workspace(void* stream);

/* ---- misc ------------------------------------------------------------------------------------------ */
const char* eetq_last_error(void);   /* thread-local, never NULL */
const char* eetq_version(void);      /* "eetq_amd <version> gfx950" */
/* 1 if the current HIP device is a gfx950; 0 otherwise (kernels are built for gfx950 only). */
int eetq_device_supported(void);

#ifdef __cplusplus
}
#endif
#endif /* EETQ_AMD_H_ */
