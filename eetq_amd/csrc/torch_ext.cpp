// The compiled operator module `EETQ`: torch::Tensor in / torch::Tensor out over the C ABI of libeetq_amd.so.
//
// Drop-in for the reference's pybind module (csrc/eetpy.cpp:7-19): the six functions it binds keep their names, argument
// order, py::arg names and defaults, current-stream / device-guard behaviour and error type (C++ exception ->
// RuntimeError).  Host code only (g++): every kernel lives behind include/eetq_amd.h.  Optional trailing keyword arguments
// (layout=, path=, bias=, residual=, norm=, gated=) and five further functions are extensions of this library
// (include/eetq_amd.h says which reference interface, if any, each one stands in for).
#include <torch/extension.h>

#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <array>
#include <cmath>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/eetq_amd.h"

namespace {

using torch::Tensor;
using OptTensor = std::optional<Tensor>;

void check(int status)
{
    if (status != EETQ_OK) {
        const char* msg = eetq_last_error();
        throw std::runtime_error(msg && *msg ? msg : "eetq_amd: error " + std::to_string(status));
    }
}

void* stream_of(const Tensor& t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

int layout_id(const std::string& name)
{
    if (name == "gfx950" || name == "native") return EETQ_LAYOUT_GFX950;
    if (name == "sm80") return EETQ_LAYOUT_SM80;
    if (name == "row_major") return EETQ_LAYOUT_ROW_MAJOR;
    throw std::runtime_error("unknown weight layout '" + name + "' (expected 'gfx950', 'sm80' or 'row_major')");
}

int path_id(const std::string& name)
{
    if (name == "auto") return EETQ_PATH_AUTO;
    if (name == "gemv") return EETQ_PATH_GEMV;
    if (name == "mfma") return EETQ_PATH_MFMA;
    if (name == "stream") return EETQ_PATH_STREAM;
    if (name == "mid") return EETQ_PATH_MID;
    if (name == "splitk") return EETQ_PATH_SPLITK;
    if (name == "tilesplit") return EETQ_PATH_TILESPLIT;
    throw std::runtime_error("unknown GEMM path '" + name + "'");
}

c10::Device work_device(const Tensor& t)
{
    if (t.is_cuda()) return t.device();
    TORCH_CHECK(torch::cuda::is_available(), "eetq_amd: no HIP device available; the W8A16 path has no CPU implementation");
    return c10::Device(c10::kCUDA, c10::hip::current_device());
}

// ---- quantise (reference: symmetric_quantize_last_axis_of_tensor, fpA_intB_gemm_wrapper.cu:28-107) ----------------
std::vector<Tensor> quant_weights(const Tensor& weight, py::object quant_type, bool return_unprocessed_quantized_tensor,
                                  const std::string& layout)
{
    const at::ScalarType qt = torch::python::detail::py_object_to_dtype(quant_type);
    TORCH_CHECK(weight.is_contiguous(), "weight must be contiguous");
    TORCH_CHECK(weight.numel() != 0, "weight should not be empty tensor");
    TORCH_CHECK(weight.dim() == 2 || weight.dim() == 3, "Invalid dim. The dim of weight should be 2 or 3");
    const auto st = weight.scalar_type();
    TORCH_CHECK(st == at::kHalf || st == at::kFloat, "Invalid datatype. Weight must be FP16 or FP32");
    TORCH_CHECK(qt == at::kChar || qt == at::kQUInt4x2, "Must be int4 or int8 quantization");
    if (weight.dim() == 3) {
        // [E, K, N] expert stack.  The reference accepts it, allocates [E, K, N] / [E, N] outputs (fpA_intB_gemm_wrapper.cu:45-66)
        // and then hands symmetric_quantize the 2-D shape {num_rows, num_cols} (:82, :90): only expert 0 is quantised, the other
        // experts' outputs stay uninitialised.  Here every expert is quantised -- the same output shapes, expert 0 identical.
        std::vector<Tensor> parts[3];
        for (int64_t e = 0; e < weight.size(0); ++e) {
            auto r = quant_weights(weight.select(0, e), quant_type, return_unprocessed_quantized_tensor, layout);
            for (size_t i = 0; i < r.size(); ++i) parts[i].push_back(r[i]);
        }
        std::vector<Tensor> out;
        for (auto& p : parts)
            if (!p.empty()) out.push_back(torch::stack(p, 0));
        return out;
    }
    const bool   int4 = qt == at::kQUInt4x2;
    const int    lay  = layout_id(layout);
    const size_t K = weight.size(0), N = weight.size(1);
    const auto   dev = work_device(weight);
    c10::DeviceGuard guard(dev);
    Tensor       w_dev = weight.is_cuda() ? weight : weight.to(dev);
    const auto   i8    = torch::TensorOptions().dtype(at::kChar).device(dev);
    Tensor       raw, processed, scales = torch::empty({(int64_t)N}, weight.options().device(dev));
    // workspace of the quantiser (int8: one row of column maxima per 128 weight rows; int4: N floats)
    Tensor colmax = torch::empty({(int64_t)(int4 ? N : eetq_quantize_workspace_floats(K, N))},
                                 torch::TensorOptions().dtype(at::kFloat).device(dev));
    if (!int4) {
        if (return_unprocessed_quantized_tensor) raw = torch::empty({(int64_t)K, (int64_t)N}, i8);
        processed = torch::empty({(int64_t)K, (int64_t)N}, i8);
        check(eetq_quantize_i8_ws(w_dev.data_ptr(), st == at::kHalf ? EETQ_DTYPE_F16 : EETQ_DTYPE_F32, K, N,
                                  raw.defined() ? raw.data_ptr<int8_t>() : nullptr, processed.data_ptr<int8_t>(), lay,
                                  scales.data_ptr(), colmax.data_ptr<float>(), (size_t)colmax.numel(), stream_of(w_dev)));
    } else {
        // packed int4: two values per byte along N (reference output shape [K, N/2], fpA_intB_gemm_wrapper.cu:60-66)
        TORCH_CHECK(N % 2 == 0, "int4 quantization needs an even number of columns");
        if (return_unprocessed_quantized_tensor) raw = torch::empty({(int64_t)K, (int64_t)N / 2}, i8);
        processed = torch::empty({(int64_t)K, (int64_t)N / 2}, i8);
        check(eetq_quantize_i4(w_dev.data_ptr(), st == at::kHalf ? EETQ_DTYPE_F16 : EETQ_DTYPE_F32, K, N,
                               raw.defined() ? raw.data_ptr<int8_t>() : nullptr, processed.data_ptr<int8_t>(), lay,
                               scales.data_ptr(), colmax.data_ptr<float>(), stream_of(w_dev)));
    }
    if (!weight.is_cuda()) {  // CPU tensors in -> CPU tensors out, like the reference (:33)
        processed = processed.cpu();
        scales    = scales.cpu();
        if (raw.defined()) raw = raw.cpu();
    }
    if (return_unprocessed_quantized_tensor) return {raw, processed, scales};
    return {processed, scales};
}

Tensor relayout(const Tensor& src_in, const std::string& layout, bool pack, bool is_int4)
{
    TORCH_CHECK(src_in.scalar_type() == at::kChar, "expected an int8 tensor");
    if (src_in.dim() != 2) throw std::runtime_error("[FT][ERROR] Shape must be 2-D");
    Tensor       src = src_in.contiguous();
    const int    lay = layout_id(layout);
    const size_t K = src.size(0), Nb = src.size(1);
    const auto   dev = work_device(src);
    c10::DeviceGuard guard(dev);
    Tensor       s_dev = src.is_cuda() ? src : src.to(dev);
    Tensor       out   = torch::empty_like(s_dev);
    if (is_int4)
        check((pack ? eetq_pack_i4 : eetq_unpack_i4)(s_dev.data_ptr<int8_t>(), K, Nb * 2, out.data_ptr<int8_t>(), lay,
                                                     stream_of(s_dev)));
    else
        check((pack ? eetq_pack_i8 : eetq_unpack_i8)(s_dev.data_ptr<int8_t>(), K, Nb, out.data_ptr<int8_t>(), lay,
                                                     stream_of(s_dev)));
    return src.is_cuda() ? out : out.cpu();
}

// reference: preprocess_weights_cuda, fpA_intB_gemm_wrapper.cu:109-128
Tensor preprocess_weights(const Tensor& origin_weight, bool is_int4, const std::string& layout)
{
    return relayout(origin_weight, layout, true, is_int4);
}

Tensor unprocess_weights(const Tensor& processed_weight, const std::string& layout, bool is_int4)
{
    return relayout(processed_weight, layout, false, is_int4);
}

// ---- fused dequant + GEMM ---------------------------------------------------------------------------------------------
void layernorm_forward(const Tensor& input, const Tensor& gamma, Tensor& out, double eps);
// kv_start of the three attention operators (the per-row first key of a left-padded batch): contiguous int64 [B] on the device
static const int64_t* kv_start_ptr(const char* name, const OptTensor& kv_start, const Tensor& query, int64_t B)
{
    if (!kv_start) return nullptr;
    TORCH_CHECK(kv_start->scalar_type() == at::kLong && kv_start->dim() == 1 && kv_start->size(0) == B && kv_start->is_contiguous() &&
                    kv_start->device() == query.device(),
                name, ": kv_start must be a contiguous int64 [B] tensor on the query's device");
    return kv_start->data_ptr<int64_t>();
}
// `ring` of the decode-attention operators (the cache tensors are rings of R = S rows): what it needs and excludes,
// as ValueErrors -- they are about the combination asked for, not about the tensors
static void check_decode_ring(const char* name, bool ring, const std::optional<int64_t>& window, const OptTensor& kv_start,
                              const OptTensor& mask, const OptTensor& kv_len, int64_t R)
{
    if (!ring) return;
    TORCH_CHECK_VALUE(window.has_value(), name, ": ring needs window (a ring cache holds the last rows of a sliding window only)");
    TORCH_CHECK_VALUE(R >= *window, name, ": a ring cache of ", R, " rows is too small for window ", *window, " (R >= window)");
    TORCH_CHECK_VALUE(!kv_start, name, ": ring and kv_start exclude each other (no ragged ring)");
    TORCH_CHECK_VALUE(!mask, name, ": ring and an additive mask exclude each other (the mask row would need the same wrap)");
    TORCH_CHECK_VALUE(kv_len.has_value(), name, ": ring needs kv_len (the valid length of a ring is logical, not its capacity)");
}
// What the four decode-attention operators prepare alike: the slots and their stride, the mask row and its batch stride, the kv_len /
// advance scalars, the default scaling and chunk count, the output and the workspace, the stride arrays.  name: "operator: "
struct DecodeAttnPrep {
    const int64_t *slots = nullptr, *kv_len;
    int64_t*       advance;
    int            slot_stride = 0;
    Tensor         mrow, out, ws;
    int64_t        m_sb = 0, splits;
    float          sc;

    DecodeAttnPrep(const char* name, const Tensor& query, int64_t S, const OptTensor* slots_in, const OptTensor& mask,
                   std::optional<double> scaling, std::optional<int64_t> splits_in, const OptTensor& kv_len_in, const OptTensor& advance_in)
    {
        const int64_t B = query.size(0), H = query.size(1), D = query.size(2);
        if (slots_in && *slots_in) {
            const Tensor& s = **slots_in;
            TORCH_CHECK(s.scalar_type() == at::kLong && s.device() == query.device() && (s.numel() == 1 || s.numel() == B) &&
                            s.is_contiguous(),
                        name, "slots must be contiguous int64 on the device, 1 or B elements");
            slots       = s.data_ptr<int64_t>();
            slot_stride = (s.numel() == B && B > 1) ? 1 : 0;
        }
        if (mask) {
            mrow = mask->dim() != 2 ? mask->reshape({mask->size(0), -1}) : *mask;
            TORCH_CHECK(mrow.scalar_type() == at::kHalf && mrow.size(-1) >= S && mrow.stride(-1) == 1 && mrow.device() == query.device(),
                        name, "mask must be additive float16 with a dense last dimension >= S");
            TORCH_CHECK(mrow.size(0) == 1 || mrow.size(0) == B, name, "the mask needs one row per batch entry (or a single shared row)");
            m_sb = (mrow.size(0) == B && B > 1) ? mrow.stride(0) : 0;
        }
        for (const OptTensor* t : std::initializer_list<const OptTensor*>{&kv_len_in, &advance_in})
            if (*t)
                TORCH_CHECK((*t)->scalar_type() == at::kLong && (*t)->numel() == 1 && (*t)->device() == query.device(), name,
                            "kv_len / advance must be a one-element int64 tensor on the query's device");
        kv_len  = kv_len_in ? kv_len_in->data_ptr<int64_t>() : nullptr;
        advance = advance_in ? advance_in->data_ptr<int64_t>() : nullptr;
        sc      = (float)(scaling ? *scaling : 1.0 / std::sqrt((double)D));
        splits  = splits_in ? *splits_in : (int64_t)eetq_decode_attention_splits((int)B, (int)H, (int)S);
        out     = torch::empty({B, H, D}, query.options());
        ws      = torch::empty({B * H * splits * (D + 4)}, query.options().dtype(at::kFloat));
    }
    const void* mask() const { return mrow.defined() ? mrow.data_ptr() : nullptr; }
    // lead (q_b, q_h of the two-launch entries; q_b, k_b, v_b of the one-launch ones), the caches' six, mask_b, out_b, out_h
    std::array<long, 12> strides(std::initializer_list<int64_t> lead, const Tensor& kc, const Tensor& vc) const
    {
        std::array<long, 12> st{};
        size_t               n = 0;
        for (int64_t v : lead) st[n++] = (long)v;
        for (const Tensor* c : {&kc, &vc})
            for (int i = 0; i < 3; ++i) st[n++] = (long)c->stride(i);
        st[n++] = (long)m_sb, st[n++] = (long)out.stride(0), st[n++] = (long)out.stride(1);
        return st;
    }
};
// eetq_rotary_neox_kvcache_f16 + eetq_decode_attention_f16 as one launch (the decode step of a static cache)
Tensor rope_decode_attention(const Tensor& positions, const Tensor& query, const Tensor& key, const Tensor& value,
                             const Tensor& cos_sin_cache, Tensor& key_cache, Tensor& value_cache, Tensor& tickets,
                             const OptTensor& slots, const OptTensor& mask, std::optional<double> scaling,
                             std::optional<int64_t> splits_in, const OptTensor& kv_len, int64_t kv_len_bias,
                             const OptTensor& advance, const OptTensor& kv_start = std::nullopt,
                             std::optional<int64_t> window = std::nullopt, bool ring = false)
{
    if (window) TORCH_CHECK_VALUE(*window >= 1, "rope_decode_attention: window must be at least 1 row (got ", *window, ")");
    check_decode_ring("rope_decode_attention", ring, window, kv_start, mask, kv_len, key_cache.dim() == 4 ? key_cache.size(2) : 0);
    for (const Tensor* t : std::initializer_list<const Tensor*>{&query, &key, &value, &cos_sin_cache, &key_cache, &value_cache})
        TORCH_CHECK(t->scalar_type() == at::kHalf, "rope_decode_attention: float16 tensors expected");
    TORCH_CHECK(positions.scalar_type() == at::kLong && positions.is_contiguous(),
                "rope_decode_attention: positions must be contiguous int64");
    TORCH_CHECK(query.dim() == 3 && key.dim() == 3 && value.dim() == 3 && key_cache.dim() == 4 &&
                    value_cache.sizes() == key_cache.sizes(),
                "rope_decode_attention: expected query [B, H, D], key / value [B, Hkv, D], caches [B, Hkv, S, D]");
    const int64_t B = query.size(0), H = query.size(1), D = query.size(2), Hkv = key.size(1), S = key_cache.size(2);
    TORCH_CHECK(key.size(0) == B && key.size(2) == D && value.sizes() == key.sizes() && key_cache.size(0) == B &&
                    key_cache.size(1) == Hkv && key_cache.size(3) == D && H % Hkv == 0 && positions.numel() == B,
                "rope_decode_attention: shape mismatch");
    for (const Tensor* t : std::initializer_list<const Tensor*>{&query, &key, &value})
        TORCH_CHECK(t->stride(-1) == 1 && t->stride(-2) == D, "rope_decode_attention: [heads, head_size] must be dense");
    TORCH_CHECK(key_cache.stride(-1) == 1 && value_cache.stride(-1) == 1 && cos_sin_cache.is_contiguous() &&
                    cos_sin_cache.size(-1) == D,
                "rope_decode_attention: cache rows must be dense and the rotation must cover the whole head (rot_dim == D)");
    TORCH_CHECK(tickets.scalar_type() == at::kInt && tickets.is_contiguous() && tickets.numel() >= B * H + 1 &&
                    tickets.device() == query.device(),
                "rope_decode_attention: tickets must be a zeroed int32 tensor of at least B * H + 1 elements on the device");
    const DecodeAttnPrep p("rope_decode_attention: ", query, S, &slots, mask, scaling, splits_in, kv_len, advance);
    const auto           strides = p.strides({query.stride(0), key.stride(0), value.stride(0)}, key_cache, value_cache);
    const int64_t*       starts  = kv_start_ptr("rope_decode_attention", kv_start, query, B);
    unsigned*            tk      = reinterpret_cast<unsigned*>(tickets.data_ptr<int32_t>());
    c10::DeviceGuard     guard(query.device());
    if (ring) {   // the windowed entry's bits, the cache rows addressed modulo S
        check(eetq_rope_decode_attention_ring_f16(
            positions.data_ptr<int64_t>(), p.slots, p.slot_stride, query.data_ptr(), key.data_ptr(), value.data_ptr(),
            cos_sin_cache.data_ptr(), (int)(cos_sin_cache.numel() / D), key_cache.data_ptr(), value_cache.data_ptr(), p.out.data_ptr(),
            p.ws.data_ptr<float>(), tk, (int)B, (int)H, (int)Hkv, (int)S, (int)D, (int)p.splits, p.sc, strides.data(), p.kv_len,
            (int)kv_len_bias, (int)std::min<int64_t>(*window, INT32_MAX), p.advance, stream_of(query)));
        return p.out;
    }
    if (window) {   // the last `window` valid rows, not below kv_start (which may be absent)
        check(eetq_rope_decode_attention_window_f16(
            positions.data_ptr<int64_t>(), p.slots, p.slot_stride, query.data_ptr(), key.data_ptr(), value.data_ptr(),
            cos_sin_cache.data_ptr(), (int)(cos_sin_cache.numel() / D), key_cache.data_ptr(), value_cache.data_ptr(), p.mask(),
            p.out.data_ptr(), p.ws.data_ptr<float>(), tk, (int)B, (int)H, (int)Hkv, (int)S, (int)D, (int)p.splits, p.sc, strides.data(),
            p.kv_len, (int)kv_len_bias, starts, (int)std::min<int64_t>(*window, INT32_MAX), p.advance, stream_of(query)));
        return p.out;
    }
    if (starts) {
        check(eetq_rope_decode_attention_padded_f16(
            positions.data_ptr<int64_t>(), p.slots, p.slot_stride, query.data_ptr(), key.data_ptr(), value.data_ptr(),
            cos_sin_cache.data_ptr(), (int)(cos_sin_cache.numel() / D), key_cache.data_ptr(), value_cache.data_ptr(), p.mask(),
            p.out.data_ptr(), p.ws.data_ptr<float>(), tk, (int)B, (int)H, (int)Hkv, (int)S, (int)D, (int)p.splits, p.sc, strides.data(),
            p.kv_len, (int)kv_len_bias, starts, p.advance, stream_of(query)));
        return p.out;
    }
    check(eetq_rope_decode_attention_bounded_f16(
        positions.data_ptr<int64_t>(), p.slots, p.slot_stride, query.data_ptr(), key.data_ptr(), value.data_ptr(),
        cos_sin_cache.data_ptr(), (int)(cos_sin_cache.numel() / D), key_cache.data_ptr(), value_cache.data_ptr(), p.mask(),
        p.out.data_ptr(), p.ws.data_ptr<float>(), tk, (int)B, (int)H, (int)Hkv, (int)S, (int)D, (int)p.splits, p.sc, strides.data(),
        p.kv_len, (int)kv_len_bias, p.advance, stream_of(query)));
    return p.out;
}

// causal attention over a prompt on the matrix cores (eetq_prefill_attention_f16): query [B, T, H, D] (any token / head strides, D
// dense), key / value cache views [B, Hkv, rows >= keys, D]; returns [B, T, H, D] contiguous
bool prefill_attention_supported(int64_t head_dim) { return eetq_prefill_attention_supported((int)head_dim) != 0; }

int64_t prefill_attention_splits(int64_t batch, int64_t heads, int64_t q_tokens, int64_t max_keys)
{
    return eetq_prefill_attention_splits((int)batch, (int)heads, (int)q_tokens, (int)max_keys);
}

// The query [B, rows, H, D] and the cache views [B, Hkv, S >= keys, D] of prefill_attention and decode_attention_rows (`rows`: the
// letter the message calls the query rows by); name: "operator: "
static void check_prompt_qkv(const char* name, char rows, const Tensor& query, const Tensor& key, const Tensor& value, int64_t keys)
{
    for (const Tensor* t : std::initializer_list<const Tensor*>{&query, &key, &value})
        TORCH_CHECK(t->scalar_type() == at::kHalf && t->is_cuda() && t->dim() == 4 && t->stride(-1) == 1 && t->device() == query.device(),
                    name, "float16 CUDA tensors [B, ", rows, ", H, D] / [B, Hkv, S, D] with a dense last dimension expected");
    const int64_t Hkv = key.size(1);
    TORCH_CHECK(key.size(0) == query.size(0) && key.size(3) == query.size(3) && value.sizes() == key.sizes() && Hkv > 0 &&
                    query.size(2) % Hkv == 0 && keys > 0 && keys <= key.size(2),
                name, "shape mismatch");
}
// What prefill_attention, prefill_attention_i8kv and decode_attention_rows prepare alike behind their own tensor checks: the kv_len
// scalar and its bias, the default scaling, the share count (None: the library's rule) and its range, the workspace (checked, or
// allocated here: capturable), the output [B, rows, H, D] and the twelve strides.  name: "operator: "; always_ws: a workspace even of
// no elements; device_form = false (prefill_attention's host form): one share, no workspace, nothing to check.
struct PromptAttnPrep {
    const int64_t* kv_len = nullptr;
    int64_t        splits = 1;
    float          sc;
    Tensor         ws, out;
    long           st[12];

    PromptAttnPrep(const char* name, const Tensor& query, const Tensor& kc, const Tensor& vc, int64_t keys, std::optional<double> scaling,
                   const OptTensor& kv_len_in, int64_t kv_len_bias, std::optional<int64_t> splits_in, const OptTensor& workspace,
                   int (*default_splits)(int B, int H, int Hkv, int rows, int keys), int (*max_splits)(),
                   size_t (*workspace_floats)(int B, int H, int rows, int D, int splits), bool always_ws, bool device_form = true)
    {
        const int64_t B = query.size(0), R = query.size(1), H = query.size(2), D = query.size(3);
        sc = (float)(scaling ? *scaling : 1.0 / std::sqrt((double)D));
        if (device_form) {
            TORCH_CHECK(kv_len_in || kv_len_bias == 0, name, "kv_len_bias needs kv_len");
            if (kv_len_in) {
                TORCH_CHECK(kv_len_in->scalar_type() == at::kLong && kv_len_in->numel() == 1 && kv_len_in->device() == query.device(), name,
                            "kv_len must be a one-element int64 tensor on the query's device");
                kv_len = kv_len_in->data_ptr<int64_t>();
            }
            splits = splits_in ? *splits_in : (int64_t)default_splits((int)B, (int)H, (int)kc.size(1), (int)R, (int)keys);
            TORCH_CHECK(splits >= 1 && splits <= max_splits(), name, "splits must lie in 1 .. ", max_splits());
            const int64_t need = (int64_t)workspace_floats((int)B, (int)H, (int)R, (int)D, (int)splits);
            if (workspace) {
                TORCH_CHECK(workspace->scalar_type() == at::kFloat && workspace->device() == query.device() && workspace->is_contiguous() &&
                                workspace->numel() >= need,
                            name, "workspace must be a contiguous float32 tensor of at least ", need, " elements on the query's device");
                ws = *workspace;
            } else if (always_ws || need > 0) {
                ws = torch::empty({need}, query.options().dtype(at::kFloat));
            }
        }
        out = torch::empty({B, R, H, D}, query.options());
        int n = 0;
        for (const Tensor* t : std::initializer_list<const Tensor*>{&query, &kc, &vc, &out})
            for (int i = 0; i < 3; ++i) st[n++] = (long)t->stride(i);
    }
    float* workspace() const { return ws.defined() ? ws.data_ptr<float>() : nullptr; }
};
static int prefill_splits_rule(int B, int H, int, int T, int keys) { return eetq_prefill_attention_splits(B, H, T, keys); }

// kv_len (a one-element int64 tensor on the query's device): `keys` is then the upper bound and the number of keys is read on the
// device (eetq_prefill_attention_dev_f16); splits: None = the library's rule, workspace: None = allocated here (capturable)
Tensor prefill_attention(const Tensor& query, const Tensor& key, const Tensor& value, int64_t keys, std::optional<double> scaling,
                         std::optional<int64_t> causal_offset, const OptTensor& kv_len, int64_t kv_len_bias,
                         std::optional<int64_t> splits_in, const OptTensor& workspace, const OptTensor& kv_start = std::nullopt,
                         std::optional<int64_t> window = std::nullopt, bool ring = false)
{
    // ring: key / value are rings of R = key.size(2) rows; `keys` and kv_len count logical rows and may exceed R
    if (ring) {
        TORCH_CHECK_VALUE(window.has_value(), "prefill_attention: ring needs window (a ring cache holds the last rows of a sliding window only)");
        TORCH_CHECK_VALUE(!causal_offset, "prefill_attention: ring takes causal_offset = keys - query rows only");
        if (key.dim() == 4 && query.dim() == 4) {
            const int64_t R = key.size(2), T = query.size(1);
            TORCH_CHECK_VALUE(R % 64 == 0, "prefill_attention: a ring cache behind the prompt kernel must have a multiple of 64 rows (got ", R,
                              ": a key block must not straddle the ring's end)");
            TORCH_CHECK_VALUE(*window >= 1 && R >= *window + T + 62, "prefill_attention: a ring cache of ", R, " rows is too small for window ",
                              *window, " and ", T, " query rows (R >= window + query rows + 62: a launch must not read key blocks its own "
                              "rows have replaced)");
        }
    }
    // the sliding window's refusals come first and are ValueErrors: they are about the combination asked for, not about the tensors
    if (window) {
        TORCH_CHECK_VALUE(*window >= 1, "prefill_attention: window must be at least 1 row (got ", *window, ")");
        TORCH_CHECK_VALUE(!kv_start, "prefill_attention: window and kv_start exclude each other (the windowed prompt kernel knows one "
                                     "shared first key; ragged prompts with a window are not built)");
    }
    check_prompt_qkv("prefill_attention: ", 'T', query, key, value, ring && key.dim() == 4 ? std::min<int64_t>(keys, key.size(2)) : keys);
    TORCH_CHECK(keys > 0 && keys <= (int64_t(1) << 30), "prefill_attention: keys out of range");
    const int64_t B = query.size(0), T = query.size(1), H = query.size(2), D = query.size(3), Hkv = key.size(1);
    TORCH_CHECK(T > 0, "prefill_attention: shape mismatch");
    TORCH_CHECK(prefill_attention_supported(D), "prefill_attention: unsupported head_dim");
    const int64_t off = causal_offset ? *causal_offset : keys - T;
    const int64_t* starts = kv_start_ptr("prefill_attention", kv_start, query, B);
    const bool   dev_form = kv_len.has_value() || splits_in.has_value() || workspace.has_value() || kv_len_bias != 0 || starts || window;
    if (dev_form)
        TORCH_CHECK(!(kv_len && causal_offset), "prefill_attention: kv_len and causal_offset exclude each other (with kv_len the offset is "
                                                "the device length minus the query rows)");
    // window: a workgroup reads at most the window and its own 128 rows' keys -- the rule sizes the shares by that (untuned)
    const int64_t rule_keys = window ? std::min<int64_t>(keys, std::min<int64_t>(*window, keys) + std::min<int64_t>(T, 128)) : keys;
    const PromptAttnPrep p("prefill_attention: ", query, key, value, rule_keys, scaling, kv_len, kv_len_bias, splits_in, workspace,
                           prefill_splits_rule, eetq_prefill_attention_max_splits, eetq_prefill_attention_workspace_floats, false, dev_form);
    c10::DeviceGuard guard(query.device());
    if (ring) {   // the windowed entry's bits, the cache rows addressed modulo key.size(2)
        check(eetq_prefill_attention_ring_f16(query.data_ptr(), key.data_ptr(), value.data_ptr(), p.out.data_ptr(), p.workspace(), (int)B,
                                              (int)H, (int)Hkv, (int)T, (int)keys, (int)D, p.kv_len, (int)kv_len_bias,
                                              (int)std::min<int64_t>(*window, INT32_MAX), (int)key.size(2), (int)p.splits, p.sc, p.st,
                                              stream_of(query)));
        return p.out;
    }
    if (window) {   // always the device-length entry (kv_len None: `keys` keys, the fresh prompt)
        TORCH_CHECK(off == keys - T, "prefill_attention: window takes causal_offset = keys - query rows only");
        check(eetq_prefill_attention_window_f16(query.data_ptr(), key.data_ptr(), value.data_ptr(), p.out.data_ptr(), p.workspace(), (int)B,
                                                (int)H, (int)Hkv, (int)T, (int)keys, (int)D, p.kv_len, (int)kv_len_bias,
                                                (int)std::min<int64_t>(*window, INT32_MAX), (int)p.splits, p.sc, p.st, stream_of(query)));
        return p.out;
    }
    if (starts) {   // the per-row first key: always the device-length entry (kv_len None: `keys` keys, the fresh prompt)
        TORCH_CHECK(off == keys - T, "prefill_attention: kv_start takes causal_offset = keys - query rows only");
        check(eetq_prefill_attention_padded_f16(query.data_ptr(), key.data_ptr(), value.data_ptr(), p.out.data_ptr(), p.workspace(), (int)B,
                                                (int)H, (int)Hkv, (int)T, (int)keys, (int)D, p.kv_len, (int)kv_len_bias, starts,
                                                (int)p.splits, p.sc, p.st, stream_of(query)));
        return p.out;
    }
    if (kv_len || p.splits > 1) {
        TORCH_CHECK(kv_len || off == keys - T, "prefill_attention: the split form takes causal_offset = keys - query rows only");
        check(eetq_prefill_attention_dev_f16(query.data_ptr(), key.data_ptr(), value.data_ptr(), p.out.data_ptr(), p.workspace(), (int)B,
                                             (int)H, (int)Hkv, (int)T, (int)keys, (int)D, p.kv_len, (int)kv_len_bias, (int)p.splits, p.sc,
                                             p.st, stream_of(query)));
        return p.out;
    }
    check(eetq_prefill_attention_f16(query.data_ptr(), key.data_ptr(), value.data_ptr(), p.out.data_ptr(), (int)B, (int)H, (int)Hkv, (int)T,
                                     (int)keys, (int)D, (int)off, p.sc, p.st, stream_of(query)));
    return p.out;
}

// 1 .. 16 query rows behind a long cache, split-KV on the matrix cores (eetq_decode_attention_rows_f16): query [B, R, H, D] (any row /
// head strides, D dense), cache views [B, Hkv, rows >= keys, D]; returns [B, R, H, D] contiguous.  The tensor checks and the
// preparation are prefill_attention's; splits: None = the library's rule, workspace: None = allocated here (capturable, nothing persistent)
int64_t decode_attention_rows_splits(int64_t batch, int64_t heads, int64_t kv_heads, int64_t rows, int64_t max_keys)
{
    return eetq_decode_attention_rows_splits((int)batch, (int)heads, (int)kv_heads, (int)rows, (int)max_keys);
}

Tensor decode_attention_rows(const Tensor& query, const Tensor& key, const Tensor& value, int64_t keys, std::optional<double> scaling,
                             const OptTensor& kv_len, int64_t kv_len_bias, std::optional<int64_t> splits_in, const OptTensor& workspace,
                             bool ring = false)
{
    // accepted only to be refused by name
    TORCH_CHECK_VALUE(!ring, "decode_attention_rows: no ring cache behind the few-row kernel (it reads rows by their logical index)");
    check_prompt_qkv("decode_attention_rows: ", 'R', query, key, value, keys);
    const int64_t B = query.size(0), R = query.size(1), H = query.size(2), D = query.size(3), Hkv = key.size(1);
    TORCH_CHECK(B > 0, "decode_attention_rows: shape mismatch");
    TORCH_CHECK(R >= 1 && R <= 16, "decode_attention_rows: 1 .. 16 query rows per batch row (got ", R, ")");
    TORCH_CHECK(D == 64 || D == 128, "decode_attention_rows: unsupported head_dim");
    const PromptAttnPrep p("decode_attention_rows: ", query, key, value, keys, scaling, kv_len, kv_len_bias, splits_in, workspace,
                           eetq_decode_attention_rows_splits, eetq_decode_attention_rows_max_splits,
                           eetq_decode_attention_rows_workspace_floats, true);
    c10::DeviceGuard guard(query.device());
    check(eetq_decode_attention_rows_f16(query.data_ptr(), key.data_ptr(), value.data_ptr(), p.out.data_ptr(), p.workspace(), (int)B, (int)H,
                                         (int)Hkv, (int)R, (int)keys, (int)D, p.kv_len, (int)kv_len_bias, (int)p.splits, p.sc, p.st,
                                         stream_of(query)));
    return p.out;
}

Tensor silu_mul(const Tensor& gate_up, bool glu8 = false);

void check_epilogue(const Tensor& input, const OptTensor& bias, const OptTensor& residual, int64_t m, int64_t n)
{
    if (bias) {
        const Tensor& b = *bias;
        TORCH_CHECK(b.scalar_type() == at::kHalf && b.device() == input.device() && b.numel() == n && b.is_contiguous(),
                    "w8_a16_gemm: bias must be a contiguous float16 [N] tensor on the input's device");
    }
    if (residual) {
        const Tensor& r = *residual;
        TORCH_CHECK(r.scalar_type() == at::kHalf && r.device() == input.device() && r.numel() == m * n &&
                        r.is_contiguous() && r.size(-1) == n,
                    "w8_a16_gemm: residual must be a contiguous float16 [..., N] tensor with the output's element count, "
                    "on the input's device");
    }
}

Tensor& gemm_launch(const Tensor& input, const Tensor& weight, const Tensor& scale, Tensor& output, int64_t m, int64_t n,
                    int64_t k, int path, const OptTensor& bias, const OptTensor& residual, int act)
{
    TORCH_CHECK(input.scalar_type() == at::kHalf, "w8_a16_gemm: input must be float16 (got ", input.scalar_type(), ")");
    TORCH_CHECK(input.is_cuda(), "input must be a CUDA tensor");
    TORCH_CHECK(weight.scalar_type() == at::kChar && scale.scalar_type() == at::kHalf,
                "w8_a16_gemm: weight must be int8 and scale float16");
    TORCH_CHECK(weight.device() == input.device() && scale.device() == input.device() && output.device() == input.device(),
                "w8_a16_gemm: input, weight, scale and output must be on the same device");
    TORCH_CHECK(weight.is_contiguous() && scale.is_contiguous() && output.is_contiguous(),
                "w8_a16_gemm: weight, scale and output must be contiguous");
    check_epilogue(input, bias, residual, m, n);
    Tensor           x = input.contiguous();
    c10::DeviceGuard guard(input.device());
    const bool       int4 = weight.size(-1) * 2 == n && weight.size(-1) != n;  // packed int4: [K, N/2] bytes
    TORCH_CHECK(!int4 || act == EETQ_ACT_IDENTITY, "w8_a16_gemm: int4 weights take no activation epilogue");
    if (int4)
        check(eetq_w4a16_gemm_ex(x.data_ptr(), weight.data_ptr<int8_t>(), scale.data_ptr(), bias ? bias->data_ptr() : nullptr,
                                 residual ? residual->data_ptr() : nullptr, output.data_ptr(), (int)m, (int)n, (int)k, path,
                                 stream_of(input)));
    else
        check(eetq_w8a16_gemm_act(x.data_ptr(), weight.data_ptr<int8_t>(), scale.data_ptr(),
                                  bias ? bias->data_ptr() : nullptr, residual ? residual->data_ptr() : nullptr,
                                  output.data_ptr(), (int)m, (int)n, (int)k, path, act, stream_of(input)));
    return output;
}

int act_id(const std::string& name)
{
    if (name.empty() || name == "identity" || name == "none") return EETQ_ACT_IDENTITY;
    if (name == "relu") return EETQ_ACT_RELU;
    if (name == "gelu") return EETQ_ACT_GELU;
    if (name == "silu") return EETQ_ACT_SILU;
    throw std::runtime_error("unknown activation '" + name + "' (identity, relu, gelu, silu; silu_glu8 for gated weights)");
}

std::vector<int64_t> out_shape(const Tensor& input, int64_t n)
{
    std::vector<int64_t> s(input.sizes().begin(), input.sizes().end());
    s.back() = n;
    return s;
}

// The M = 1 GEMV stages its activation row in LDS: 65536 values at most (gemv.hip::lds_stages).  The entry points that fuse a norm, a
// gated activation or the glu8 write-out into that launch refuse a deeper row; w8_a16_gemm then runs the unfused sequence, whose
// projection AUTO puts on the small-batch kernel.
constexpr int64_t kGemvMaxStaged = 65536;

// reference: w8_a16_gemm_forward_cuda, fpA_intB_gemm_wrapper.cu:130-173 (fresh output, current stream, asynchronous)
Tensor w8_a16_gemm(const Tensor& input_in, const Tensor& weight, const Tensor& scale, const std::string& path,
                   const OptTensor& bias, const OptTensor& residual, const std::optional<std::tuple<Tensor, double>>& norm,
                   bool gated, const std::string& activation)
{
    Tensor  input = input_in;
    int64_t n     = scale.numel();  // [N]; for packed int4 weights the byte tensor is [K, N/2]
    TORCH_CHECK(input.dim() >= 1 && weight.dim() == 2, "w8_a16_gemm: expected input [..., K] and weight [K, N]");
    const int64_t kw = weight.size(0);
    if (activation == "silu_glu8") {
        // gated MLP over a weight in "glu8" column order: [..., N/2] = silu_mul of the column pairs.  One launch for a single
        // row (activation in the GEMV epilogue, RMS-norm in its prologue); projection + eetq_silu_mul_glu8_f16 otherwise.
        TORCH_CHECK(!gated && !residual && n % 16 == 0 && weight.size(1) == n,
                    "w8_a16_gemm: silu_glu8 takes an int8 [K, N] weight with N % 16 == 0, no residual");
        const int64_t rows = kw ? input.numel() / kw : 0;
        const bool    fusable_norm = !norm || (std::get<0>(*norm).scalar_type() == at::kHalf &&
                                            std::get<0>(*norm).is_contiguous() && std::get<0>(*norm).numel() == kw &&
                                            std::get<0>(*norm).device() == input.device());
        if (rows == 1 && path == "auto" && kw <= kGemvMaxStaged && input.size(-1) == kw && input.is_cuda() &&
            input.scalar_type() == at::kHalf && fusable_norm) {
            TORCH_CHECK(weight.scalar_type() == at::kChar && scale.scalar_type() == at::kHalf && weight.is_contiguous() &&
                            weight.device() == input.device() && scale.device() == input.device(),
                        "w8_a16_gemm: weight must be contiguous int8 and scale float16, on the input's device");
            check_epilogue(input, bias, residual, 1, n);
            Tensor           x = input.contiguous();
            Tensor           output = torch::empty(out_shape(input, n / 2), input.options());
            c10::DeviceGuard guard(input.device());
            check(eetq_w8a16_gemv_glu8(x.data_ptr(), norm ? std::get<0>(*norm).data_ptr() : nullptr,
                                       norm ? (float)std::get<1>(*norm) : 0.f, weight.data_ptr<int8_t>(), scale.data_ptr(),
                                       bias ? bias->data_ptr() : nullptr, output.data_ptr(), (int)n, (int)kw, stream_of(input)));
            return output;
        }
        if (rows >= 2 && rows <= 16 && path == "auto" && input.size(-1) == kw && input.is_cuda() &&
            input.scalar_type() == at::kHalf && weight.scalar_type() == at::kChar && scale.scalar_type() == at::kHalf &&
            weight.is_contiguous() && weight.device() == input.device() && scale.device() == input.device()) {
            // batched decode: the activation in the stream kernel's epilogue (the norm, if any, as its own launch first)
            Tensor xin = input.contiguous();
            if (norm) {
                Tensor normed = torch::empty_like(xin);
                layernorm_forward(xin, std::get<0>(*norm), normed, std::get<1>(*norm));
                xin = normed;
            }
            check_epilogue(input, bias, residual, rows, n);
            Tensor           output = torch::empty(out_shape(input, n / 2), input.options());
            c10::DeviceGuard guard(input.device());
            check(eetq_w8a16_gemm_glu8(xin.data_ptr(), weight.data_ptr<int8_t>(), scale.data_ptr(),
                                       bias ? bias->data_ptr() : nullptr, output.data_ptr(), (int)rows, (int)n, (int)kw,
                                       stream_of(input)));
            return output;
        }
        if (rows > 16 && path == "auto" && input.size(-1) == kw && input.is_cuda() && input.scalar_type() == at::kHalf &&
            weight.scalar_type() == at::kChar && scale.scalar_type() == at::kHalf && weight.is_contiguous() &&
            weight.device() == input.device() && scale.device() == input.device()) {
            // prompts: the tiled MFMA kernel writes the activation out of its fp16 tile image where AUTO runs the shape on it
            Tensor xin = input.contiguous();
            if (norm) {
                Tensor normed = torch::empty_like(xin);
                layernorm_forward(xin, std::get<0>(*norm), normed, std::get<1>(*norm));
                xin = normed;
            }
            check_epilogue(input, bias, residual, rows, n);
            Tensor           output = torch::empty(out_shape(input, n / 2), input.options());
            c10::DeviceGuard guard(input.device());
            const int        st = eetq_w8a16_gemm_glu8(xin.data_ptr(), weight.data_ptr<int8_t>(), scale.data_ptr(),
                                                       bias ? bias->data_ptr() : nullptr, output.data_ptr(), (int)rows, (int)n,
                                                       (int)kw, stream_of(input));
            if (st != EETQ_ERR_UNSUPPORTED) {
                check(st);
                return output;
            }
            return silu_mul(w8_a16_gemm(xin, weight, scale, path, bias, residual, std::nullopt, false, std::string()), true);
        }
        return silu_mul(w8_a16_gemm(input_in, weight, scale, path, bias, residual, norm, false, std::string()), true);
    }
    if (gated) {
        TORCH_CHECK(input.size(-1) == 2 * kw, "w8_a16_gemm: gated input must be [..., 2K] for a [K, N] weight");
        const int64_t rows = input.numel() / input.size(-1);
        if (rows == 1 && path == "auto" && kw <= kGemvMaxStaged && !norm && input.is_cuda() && input.scalar_type() == at::kHalf &&
            input.is_contiguous() && kw % 8 == 0 && weight.size(1) == n && activation.empty()) {
            TORCH_CHECK(weight.scalar_type() == at::kChar && scale.scalar_type() == at::kHalf && weight.is_contiguous(),
                        "w8_a16_gemm: weight must be contiguous int8 and scale float16");
            Tensor output = torch::empty(out_shape(input, n), input.options());
            check_epilogue(input, bias, residual, 1, n);
            c10::DeviceGuard guard(input.device());
            check(eetq_w8a16_gemv_silu_gated(input.data_ptr(), weight.data_ptr<int8_t>(), scale.data_ptr(),
                                             bias ? bias->data_ptr() : nullptr, residual ? residual->data_ptr() : nullptr,
                                             output.data_ptr(), (int)n, (int)kw, stream_of(input)));
            return output;
        }
        input = silu_mul(input.contiguous());
    }
    const int64_t k = input.size(-1);
    TORCH_CHECK(kw == k, "w8_a16_gemm: weight is [", kw, ", ", n, "] but input has K=", k);
    const int64_t m      = k ? input.numel() / k : 0;
    Tensor        output = torch::empty(out_shape(input, n), input.options());
    if (m == 0) return output;
    if (norm) {
        const Tensor& gamma = std::get<0>(*norm);
        const double  eps   = std::get<1>(*norm);
        if (m == 1 && path == "auto" && k <= kGemvMaxStaged && gamma.scalar_type() == at::kHalf && gamma.is_contiguous() &&
            gamma.numel() == k && weight.size(1) == n && activation.empty()) {
            TORCH_CHECK(input.scalar_type() == at::kHalf && input.is_cuda(), "w8_a16_gemm: input must be a float16 CUDA tensor");
            TORCH_CHECK(weight.scalar_type() == at::kChar && scale.scalar_type() == at::kHalf && weight.is_contiguous(),
                        "w8_a16_gemm: weight must be contiguous int8 and scale float16");
            TORCH_CHECK(gamma.device() == input.device() && weight.device() == input.device() &&
                            scale.device() == input.device(),
                        "w8_a16_gemm: all tensors must be on the input's device");
            check_epilogue(input, bias, residual, 1, n);
            Tensor           x = input.contiguous();
            c10::DeviceGuard guard(input.device());
            check(eetq_w8a16_gemv_rmsnorm(x.data_ptr(), gamma.data_ptr(), (float)eps, weight.data_ptr<int8_t>(),
                                          scale.data_ptr(), bias ? bias->data_ptr() : nullptr,
                                          residual ? residual->data_ptr() : nullptr, output.data_ptr(), (int)n, (int)k,
                                          stream_of(input)));
            return output;
        }
        Tensor xin    = input.contiguous();
        Tensor normed = torch::empty_like(xin);
        layernorm_forward(xin, gamma, normed, eps);
        input = normed;
    }
    return gemm_launch(input, weight, scale, output, m, n, k, path_id(path), bias, residual, act_id(activation));
}

// reference: w8_a16_gemm_forward_cuda_, fpA_intB_gemm_wrapper.cu:176-202 (writes into `output`, returns it)
Tensor w8_a16_gemm_(const Tensor& input, const Tensor& weight, const Tensor& scale, Tensor& output, int64_t m, int64_t n,
                    int64_t k)
{
    return gemm_launch(input, weight, scale, output, m, n, k, EETQ_PATH_AUTO, std::nullopt, std::nullopt, EETQ_ACT_IDENTITY);
}

// Extension: the projection's input gradient, out[..., K] = input[..., N] . fp16(q s)^T (eetq_w8a16_gemm_t): what the reference's
// EetqLinearMMFunction.backward computes as grad @ W_deq^T (python/eetq/modules/qlinear.py:80-94) after dequantising W through
// an identity GEMM.  Fresh output, current stream, asynchronous; every argument check comes before any GPU work.
Tensor w8_a16_gemm_t(const Tensor& input, const Tensor& weight, const Tensor& scale)
{
    TORCH_CHECK(input.is_cuda() && weight.is_cuda() && scale.is_cuda(), "w8_a16_gemm_t: input, weight and scale must be GPU tensors");
    TORCH_CHECK(input.scalar_type() == at::kHalf, "w8_a16_gemm_t: input must be float16 (got ", input.scalar_type(), ")");
    TORCH_CHECK(weight.dim() == 2 && weight.scalar_type() == at::kChar && scale.scalar_type() == at::kHalf,
                "w8_a16_gemm_t: weight must be an int8 [K, N] tensor and scale float16");
    TORCH_CHECK(weight.device() == input.device() && scale.device() == input.device(),
                "w8_a16_gemm_t: input, weight and scale must be on the same device");
    const int64_t k = weight.size(0), n = weight.size(1);
    TORCH_CHECK(n == 0 || scale.numel() != 2 * n, "w8_a16_gemm_t: packed int4 weights are not supported (int8 only)");
    TORCH_CHECK(scale.numel() == n, "w8_a16_gemm_t: scale must have N = ", n, " elements (got ", scale.numel(), ")");
    TORCH_CHECK(input.dim() >= 1 && input.size(-1) == n, "w8_a16_gemm_t: weight is [", k, ", ", n, "] but input has N=",
                input.dim() >= 1 ? input.size(-1) : 0);
    TORCH_CHECK(weight.is_contiguous() && scale.is_contiguous(), "w8_a16_gemm_t: weight and scale must be contiguous");
    std::vector<int64_t> shape(input.sizes().begin(), input.sizes().end());
    shape.back()        = k;
    Tensor        output = torch::empty(shape, input.options());
    const int64_t m      = n ? input.numel() / n : 0;
    if (m == 0 || k == 0) return output;
    TORCH_CHECK(m <= INT32_MAX, "w8_a16_gemm_t: too many rows");
    Tensor x = input.contiguous();  // a stride-0 gradient (y.sum().backward()) is materialised here
    if (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 != 0) x = x.clone();
    c10::DeviceGuard guard(input.device());
    check(eetq_w8a16_gemm_t(x.data_ptr(), weight.data_ptr(), scale.data_ptr(), output.data_ptr(), (int)m, (int)n, (int)k,
                            stream_of(input)));
    return output;
}

// The same from a packed int4 [K, N/2] weight in the gfx950 int4 layout (eetq_w4a16_gemm_t): the input gradient of W4A16Linear,
// the bits of w8_a16_gemm_t on the same integers held as int8.  Checks as above, all before any GPU work.
Tensor w4_a16_gemm_t(const Tensor& input, const Tensor& weight, const Tensor& scale)
{
    TORCH_CHECK(input.is_cuda() && weight.is_cuda() && scale.is_cuda(), "w4_a16_gemm_t: input, weight and scale must be GPU tensors");
    TORCH_CHECK(input.scalar_type() == at::kHalf, "w4_a16_gemm_t: input must be float16 (got ", input.scalar_type(), ")");
    TORCH_CHECK(weight.dim() == 2 && weight.scalar_type() == at::kChar && scale.scalar_type() == at::kHalf,
                "w4_a16_gemm_t: weight must be an int8 [K, N/2] tensor (packed int4) and scale float16");
    TORCH_CHECK(weight.device() == input.device() && scale.device() == input.device(),
                "w4_a16_gemm_t: input, weight and scale must be on the same device");
    const int64_t k = weight.size(0), half = weight.size(1), n = 2 * half;
    TORCH_CHECK(half == 0 || scale.numel() != half,
                "w4_a16_gemm_t: weight must be packed int4 [K, N/2] (got an int8 [K, N] weight with N scales: that is w8_a16_gemm_t's)");
    TORCH_CHECK(scale.numel() == n, "w4_a16_gemm_t: scale must have N = ", n, " elements (got ", scale.numel(), ")");
    TORCH_CHECK(input.dim() >= 1 && input.size(-1) == n, "w4_a16_gemm_t: weight is [", k, ", ", n, " / 2] but input has N=",
                input.dim() >= 1 ? input.size(-1) : 0);
    TORCH_CHECK(k % 128 == 0 && n % 16 == 0, "w4_a16_gemm_t: the int4 layout needs K % 128 == 0 and N % 16 == 0 (got K=", k, ", N=", n,
                ")");
    TORCH_CHECK(weight.is_contiguous() && scale.is_contiguous(), "w4_a16_gemm_t: weight and scale must be contiguous");
    std::vector<int64_t> shape(input.sizes().begin(), input.sizes().end());
    shape.back()        = k;
    Tensor        output = torch::empty(shape, input.options());
    const int64_t m      = n ? input.numel() / n : 0;
    if (m == 0 || k == 0) return output;
    TORCH_CHECK(m <= INT32_MAX, "w4_a16_gemm_t: too many rows");
    Tensor x = input.contiguous();  // a stride-0 gradient (y.sum().backward()) is materialised here
    if (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 != 0) x = x.clone();
    c10::DeviceGuard guard(input.device());
    check(eetq_w4a16_gemm_t(x.data_ptr(), weight.data_ptr(), scale.data_ptr(), output.data_ptr(), (int)m, (int)n, (int)k,
                            stream_of(input)));
    return output;
}

// Extension: the prompt path of a W4A16 projection on the int4 tiles themselves (eetq_w4a16_gemm_tiled): the bits of
// w8_a16_gemm(path="mfma")'s unsplit tile without the expansion to int8 tiles and its per-stream scratch.  The tensor checks are
// w8_a16_gemm's for a packed int4 weight, all before any GPU work; fresh output, current stream, asynchronous.  tile: 0 = the
// launcher's rule, 1 = 128 x 64, 2 = 128 x 128.  A shape outside w4_a16_gemm_tiled_supported raises.
bool w4_a16_gemm_tiled_supported(int64_t M, int64_t N, int64_t K)
{
    if (M < 1 || N < 1 || K < 1 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX) return false;
    return eetq_w4a16_gemm_tiled_supported((int)M, (int)N, (int)K) == 1;
}

Tensor w4_a16_gemm_tiled(const Tensor& input, const Tensor& weight, const Tensor& scale, const OptTensor& bias,
                         const OptTensor& residual, int64_t tile)
{
    TORCH_CHECK(input.scalar_type() == at::kHalf, "w4_a16_gemm_tiled: input must be float16 (got ", input.scalar_type(), ")");
    TORCH_CHECK(input.is_cuda(), "w4_a16_gemm_tiled: input must be a CUDA tensor");
    TORCH_CHECK(weight.dim() == 2 && weight.scalar_type() == at::kChar && scale.scalar_type() == at::kHalf,
                "w4_a16_gemm_tiled: weight must be an int8 [K, N/2] tensor (packed int4) and scale float16");
    TORCH_CHECK(weight.device() == input.device() && scale.device() == input.device(),
                "w4_a16_gemm_tiled: input, weight and scale must be on the same device");
    TORCH_CHECK(weight.is_contiguous() && scale.is_contiguous(), "w4_a16_gemm_tiled: weight and scale must be contiguous");
    const int64_t k = weight.size(0), n = scale.numel();
    TORCH_CHECK(weight.size(1) * 2 == n && n > 0,
                "w4_a16_gemm_tiled: weight must be packed int4 [K, N/2] with N scales (got [", k, ", ", weight.size(1), "] and ", n,
                " scales)");
    TORCH_CHECK(input.dim() >= 1 && input.size(-1) == k, "w4_a16_gemm_tiled: weight is [", k, ", ", n, " / 2] but input has K=",
                input.dim() >= 1 ? input.size(-1) : 0);
    TORCH_CHECK(tile >= 0 && tile <= 2, "w4_a16_gemm_tiled: tile is 0 (the launcher's rule), 1 (128 x 64) or 2 (128 x 128)");
    const int64_t m = k ? input.numel() / k : 0;
    if (bias) {
        const Tensor& b = *bias;
        TORCH_CHECK(b.scalar_type() == at::kHalf && b.device() == input.device() && b.numel() == n && b.is_contiguous(),
                    "w4_a16_gemm_tiled: bias must be a contiguous float16 [N] tensor on the input's device");
    }
    if (residual) {
        const Tensor& r = *residual;
        TORCH_CHECK(r.scalar_type() == at::kHalf && r.device() == input.device() && r.numel() == m * n && r.is_contiguous() &&
                        r.size(-1) == n,
                    "w4_a16_gemm_tiled: residual must be a contiguous float16 [..., N] tensor with the output's element count, on the "
                    "input's device");
    }
    Tensor output = torch::empty(out_shape(input, n), input.options());
    if (m == 0) return output;
    TORCH_CHECK(w4_a16_gemm_tiled_supported(m, n, k), "w4_a16_gemm_tiled: unsupported shape M=", m, ", N=", n, ", K=", k,
                ": needs N % 16 == 0, K % 128 == 0, K >= 384, N * K / 2 < 2^31 and 128 rows of input below 2 GiB (w8_a16_gemm takes "
                "the others)");
    Tensor x = input.contiguous();
    if (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 != 0) x = x.clone();
    c10::DeviceGuard guard(input.device());
    check(eetq_w4a16_gemm_tiled(x.data_ptr(), weight.data_ptr<int8_t>(), scale.data_ptr(), bias ? bias->data_ptr() : nullptr,
                                residual ? residual->data_ptr() : nullptr, output.data_ptr(), (int)m, (int)n, (int)k, (int)tile,
                                stream_of(input)));
    return output;
}

// ---- side ops ---------------------------------------------------------------------------------------------------------
// reference: layernorm_forward_cuda, layernorm.cu:98-113 (returns void; current stream here, default stream there)
void layernorm_forward(const Tensor& input, const Tensor& gamma, Tensor& out, double eps)
{
    TORCH_CHECK(input.scalar_type() == at::kHalf && gamma.scalar_type() == at::kHalf && out.scalar_type() == at::kHalf,
                "layernorm_forward: expected scalar type Half");
    TORCH_CHECK(input.is_cuda() && gamma.is_cuda() && out.is_cuda(), "layernorm_forward: tensors must be CUDA tensors");
    TORCH_CHECK(input.is_contiguous() && gamma.is_contiguous() && out.is_contiguous(),
                "layernorm_forward: tensors must be contiguous");
    const int64_t cols = input.size(-1);
    const int64_t rows = cols ? input.numel() / cols : 0;
    TORCH_CHECK(gamma.numel() == cols && out.numel() == input.numel(), "layernorm_forward: shape mismatch");
    c10::DeviceGuard guard(input.device());
    check(eetq_rmsnorm_f16(input.data_ptr(), gamma.data_ptr(), out.data_ptr(), (float)eps, (int)rows, (int)cols,
                           stream_of(input)));
}

// reference: rotary_embedding_neox, pos_encoding_kernels.cu:55-87 (float / double / half; bf16 is out of scope)
// Every rotary operator here hands the table's row count on: a token whose position is outside [0, cos_sin_cache.size(0)) is left
// unrotated (the cache-writing forms drop it: nothing rotated, nothing cached) and counted (decode_dropped_steps) -- the
// reference reads past its table there.  (rope_decode_attention hands it on too, but its kernel checks no upper bound yet:
// INTEGRATION.md.)
void rotary_embedding_neox(const Tensor& positions, Tensor& query, Tensor& key, int64_t head_size, const Tensor& cos_sin_cache)
{
    const auto st = query.scalar_type();
    TORCH_CHECK(st == at::kHalf || st == at::kFloat || st == at::kDouble,
                "eetq_amd: rotary_embedding_neox is implemented for float16, float32 and float64");
    TORCH_CHECK(key.scalar_type() == st && cos_sin_cache.scalar_type() == st,
                "rotary_embedding_neox: query, key and cos_sin_cache must share one dtype");
    TORCH_CHECK(positions.scalar_type() == at::kLong, "rotary_embedding_neox: positions must be int64");
    TORCH_CHECK(query.is_contiguous() && key.is_contiguous() && cos_sin_cache.is_contiguous() && positions.is_contiguous(),
                "rotary_embedding_neox: tensors must be contiguous");
    TORCH_CHECK(query.dim() >= 3, "rotary_embedding_neox: query must be [batch, seq, heads, head_size] or [tokens, heads, head_size]");
    const int64_t tokens = positions.numel();
    const int64_t heads  = query.size(-2);
    c10::DeviceGuard guard(query.device());
    const int dt = st == at::kHalf ? EETQ_DTYPE_F16 : (st == at::kFloat ? EETQ_DTYPE_F32 : EETQ_DTYPE_F64);
    check(eetq_rotary_neox_bounded(positions.data_ptr<int64_t>(), query.data_ptr(), key.data_ptr(), cos_sin_cache.data_ptr(),
                                   (int)cos_sin_cache.size(0), dt, (int)tokens, (int)heads, (int)head_size,
                                   (int)cos_sin_cache.size(1), stream_of(query)));
}

// tokens / heads / token stride of a [..., heads, head_size] view whose leading dimensions collapse to one stride
std::tuple<int64_t, int64_t, int64_t> token_view(const Tensor& t, int64_t head_size)
{
    TORCH_CHECK(t.dim() >= 2, "rotary_embedding_neox_strided: expected [..., heads, head_size]");
    const int64_t heads = t.size(-2), hs = t.size(-1);
    TORCH_CHECK(hs == head_size && t.stride(-1) == 1 && t.stride(-2) == hs,
                "rotary_embedding_neox_strided: the last two dimensions must be dense [heads, head_size]");
    int64_t tokens = 1, stride = -1, expect = -1;
    for (int64_t d = t.dim() - 3; d >= 0; --d) {
        tokens *= t.size(d);
        if (t.size(d) == 1) continue;
        if (stride < 0) {
            stride = t.stride(d);
            expect = stride * t.size(d);
        } else {
            TORCH_CHECK(t.stride(d) == expect, "rotary_embedding_neox_strided: leading dimensions do not collapse to one stride");
            expect = t.stride(d) * t.size(d);
        }
    }
    return {tokens, heads, stride >= 0 ? stride : heads * hs};
}

void rotary_embedding_neox_strided(const Tensor& positions, Tensor& query, Tensor& key, int64_t head_size,
                                   const Tensor& cos_sin_cache)
{
    TORCH_CHECK(query.scalar_type() == at::kHalf && key.scalar_type() == at::kHalf && cos_sin_cache.scalar_type() == at::kHalf,
                "eetq_amd: rotary_embedding_neox is implemented for float16 only");
    TORCH_CHECK(positions.scalar_type() == at::kLong && positions.is_contiguous() && cos_sin_cache.is_contiguous(),
                "rotary_embedding_neox_strided: positions must be contiguous int64, the cache contiguous");
    auto [tq, hq, sq] = token_view(query, head_size);
    auto [tk, hk, sk] = token_view(key, head_size);
    TORCH_CHECK(tq == tk && positions.numel() == tq,
                "rotary_embedding_neox_strided: query, key and positions disagree on the token count");
    c10::DeviceGuard guard(query.device());
    check(eetq_rotary_neox_strided_bounded_f16(positions.data_ptr<int64_t>(), query.data_ptr(), key.data_ptr(),
                                               cos_sin_cache.data_ptr(), (int)cos_sin_cache.size(0), (int)tq, (int)hq, (int)hk,
                                               (int)head_size, (int)cos_sin_cache.size(1), (int)sq, (int)sk, stream_of(query)));
}

void rotary_embedding_neox_kvcache(const Tensor& positions, Tensor& query, const Tensor& key, const Tensor& value,
                                   int64_t head_size, const Tensor& cos_sin_cache, Tensor& key_cache, Tensor& value_cache,
                                   const OptTensor& slots, bool ring = false)
{
    for (const Tensor* t : std::initializer_list<const Tensor*>{&query, &key, &value, &cos_sin_cache, &key_cache, &value_cache})
        TORCH_CHECK(t->scalar_type() == at::kHalf, "rotary_embedding_neox_kvcache: float16 tensors expected");
    TORCH_CHECK(positions.scalar_type() == at::kLong && positions.is_contiguous(),
                "rotary_embedding_neox_kvcache: positions must be contiguous int64");
    TORCH_CHECK(query.dim() == 3 && key.dim() == 3 && value.dim() == 3 && key_cache.dim() == 4,
                "rotary_embedding_neox_kvcache: shape mismatch");
    const int64_t B = query.size(0), H = query.size(1), D = query.size(2), Hkv = key.size(1);
    TORCH_CHECK(key.size(0) == B && key.size(2) == D && value.sizes() == key.sizes() && D == head_size &&
                    key_cache.size(0) == B && key_cache.size(1) == Hkv && key_cache.size(3) == D &&
                    value_cache.sizes() == key_cache.sizes() && value_cache.strides() == key_cache.strides() &&
                    positions.numel() == B,
                "rotary_embedding_neox_kvcache: shape mismatch");
    for (const Tensor* t : std::initializer_list<const Tensor*>{&query, &key, &value})
        TORCH_CHECK(t->stride(-1) == 1 && t->stride(-2) == D, "rotary_embedding_neox_kvcache: [heads, head_size] must be dense");
    TORCH_CHECK(key_cache.stride(-1) == 1 && cos_sin_cache.is_contiguous(), "rotary_embedding_neox_kvcache: cache rows must be dense");
    int slot_stride = 0;
    if (slots) {
        const Tensor& s = *slots;
        TORCH_CHECK(s.scalar_type() == at::kLong && s.device() == query.device() && (s.numel() == 1 || s.numel() == B) &&
                        s.is_contiguous(),
                    "rotary_embedding_neox_kvcache: slots must be contiguous int64 on the device, 1 or B elements");
        slot_stride = (s.numel() == B && B > 1) ? 1 : 0;
    }
    const long strides[6] = {(long)query.stride(0), (long)key.stride(0), (long)value.stride(0), (long)key_cache.stride(0),
                             (long)key_cache.stride(1), (long)key_cache.stride(2)};
    c10::DeviceGuard guard(query.device());
    if (ring) {   // the caches are rings of key_cache.size(2) rows: the slot counts the sequence's tokens, the row is slot mod rows
        check(eetq_rotary_neox_kvcache_ring_f16(positions.data_ptr<int64_t>(), slots ? slots->data_ptr<int64_t>() : nullptr, slot_stride,
                                                query.data_ptr(), key.data_ptr(), value.data_ptr(), cos_sin_cache.data_ptr(),
                                                (int)cos_sin_cache.size(0), key_cache.data_ptr(), value_cache.data_ptr(), (int)B, (int)H,
                                                (int)Hkv, (int)head_size, (int)cos_sin_cache.size(1), strides, (int)key_cache.size(2),
                                                stream_of(query)));
        return;
    }
    check(eetq_rotary_neox_kvcache_bounded_f16(positions.data_ptr<int64_t>(), slots ? slots->data_ptr<int64_t>() : nullptr,
                                               slot_stride, query.data_ptr(), key.data_ptr(), value.data_ptr(),
                                               cos_sin_cache.data_ptr(), (int)cos_sin_cache.size(0), key_cache.data_ptr(),
                                               value_cache.data_ptr(), (int)B, (int)H, (int)Hkv, (int)head_size,
                                               (int)cos_sin_cache.size(1), strides, (int)key_cache.size(2), stream_of(query)));
}

// What the two cache-writing prompt rotary operators prepare alike: the float16 and device checks (f16_caches: of the caches as well),
// positions, the 4-D shapes, first_row / first_row_dev, the one-token-stride rule and the six strides.  cache_check(B, Hkv, D) is the
// form's own check of its caches; name: "operator: "
struct RotaryPrefillPrep {
    int64_t        B, T, H, Hkv;
    const int64_t* first_row_dev = nullptr;
    long           strides[6];
};
template <class CacheCheck>
RotaryPrefillPrep rotary_prefill_prep(const char* name, bool f16_caches, const Tensor& positions, const Tensor& query, const Tensor& key,
                                      const Tensor& value, int64_t head_size, const Tensor& cos_sin_cache, const Tensor& key_cache,
                                      const Tensor& value_cache, int64_t first_row, const OptTensor& first_row_dev, CacheCheck cache_check,
                                      bool ring = false)
{
    const Tensor* halves[6] = {&query, &key, &value, &cos_sin_cache, &key_cache, &value_cache};
    for (int i = 0; i < (f16_caches ? 6 : 4); ++i) {
        TORCH_CHECK(halves[i]->scalar_type() == at::kHalf, name,
                    f16_caches ? "float16 tensors expected" : "float16 query, key, value and cos|sin table expected");
        TORCH_CHECK(halves[i]->is_cuda() && halves[i]->device() == query.device(), name, "all tensors must be on one CUDA device");
    }
    TORCH_CHECK(positions.scalar_type() == at::kLong && positions.is_contiguous() && positions.device() == query.device(), name,
                "positions must be contiguous int64 on the device");
    TORCH_CHECK(query.dim() == 4 && key.dim() == 4 && value.dim() == 4 && key_cache.dim() == 4, name, "shape mismatch");
    RotaryPrefillPrep p;
    p.B = query.size(0), p.T = query.size(1), p.H = query.size(2), p.Hkv = key.size(2);
    const int64_t B = p.B, T = p.T, D = query.size(3);
    cache_check(B, p.Hkv, D);
    TORCH_CHECK(key.size(0) == B && key.size(1) == T && key.size(3) == D && value.sizes() == key.sizes() && D == head_size &&
                    value_cache.strides() == key_cache.strides() && positions.numel() == B * T && first_row >= 0 &&
                    (ring ? T <= key_cache.size(2) : (first_row_dev || first_row + T <= key_cache.size(2))),
                name, "shape mismatch");
    if (first_row_dev) {
        TORCH_CHECK(first_row_dev->scalar_type() == at::kLong && first_row_dev->numel() == 1 &&
                        first_row_dev->device() == query.device(),
                    name, "first_row_dev must be one int64 on the device");
        p.first_row_dev = first_row_dev->data_ptr<int64_t>();
    }
    for (const Tensor* t : std::initializer_list<const Tensor*>{&query, &key, &value})
        TORCH_CHECK(t->stride(-1) == 1 && t->stride(-2) == D && (B == 1 || T == 1 || t->stride(0) == T * t->stride(1)), name,
                    "[heads, head_size] must be dense and the tokens of all rows one stride apart");
    const int tdim = T == 1 ? 0 : 1;  // (a size-1 dimension's stride is arbitrary)
    TORCH_CHECK((!f16_caches || key_cache.stride(-1) == 1) && cos_sin_cache.is_contiguous(), name,
                f16_caches ? "cache rows must be dense" : "the cos|sin table must be contiguous");
    for (int i = 0; i < 3; ++i) p.strides[i] = (long)halves[i]->stride(tdim), p.strides[3 + i] = (long)key_cache.stride(i);
    return p;
}

// Prefill on a pre-allocated KV cache (extension): query [B, T, H, D] rotated in place, key [B, T, Hkv, D] rotated into
// key_cache[b, :, base + t], value copied to value_cache[b, :, base + t], base = first_row_dev (device int64) or first_row:
// eetq_rotary_neox_kvcache_prefill_f16
void rotary_embedding_neox_kvcache_prefill(const Tensor& positions, Tensor& query, const Tensor& key, const Tensor& value,
                                           int64_t head_size, const Tensor& cos_sin_cache, Tensor& key_cache,
                                           Tensor& value_cache, int64_t first_row, const OptTensor& first_row_dev, bool ring = false)
{
    const char* name = "rotary_embedding_neox_kvcache_prefill: ";
    const auto  p    = rotary_prefill_prep(name, true, positions, query, key, value, head_size, cos_sin_cache, key_cache, value_cache, first_row,
                                           first_row_dev, [&](int64_t B, int64_t Hkv, int64_t D) {
                                           TORCH_CHECK(key_cache.size(0) == B && key_cache.size(1) == Hkv && key_cache.size(3) == D &&
                                                           value_cache.sizes() == key_cache.sizes(),
                                                       name, "shape mismatch");
                                       }, ring);
    c10::DeviceGuard guard(query.device());
    if (ring) {   // rows (base + t) mod key_cache.size(2)
        check(eetq_rotary_neox_kvcache_prefill_ring_f16(
            positions.data_ptr<int64_t>(), query.data_ptr(), key.data_ptr(), value.data_ptr(), cos_sin_cache.data_ptr(),
            (int)cos_sin_cache.size(0), key_cache.data_ptr(), value_cache.data_ptr(), (int)p.B, (int)p.T, p.first_row_dev, (int)first_row,
            (int)p.H, (int)p.Hkv, (int)head_size, (int)cos_sin_cache.size(1), p.strides, (int)key_cache.size(2), stream_of(query)));
        return;
    }
    check(eetq_rotary_neox_kvcache_prefill_bounded_f16(
        positions.data_ptr<int64_t>(), query.data_ptr(), key.data_ptr(), value.data_ptr(), cos_sin_cache.data_ptr(),
        (int)cos_sin_cache.size(0), key_cache.data_ptr(), value_cache.data_ptr(), (int)p.B, (int)p.T, p.first_row_dev, (int)first_row,
        (int)p.H, (int)p.Hkv, (int)head_size, (int)cos_sin_cache.size(1), p.strides, (int)key_cache.size(2), stream_of(query)));
}

// Greedy decode hand-over (extension): argmax of logits [B, V] (fp16, dense rows) -> out_tokens[:, column] and next_token, then
// position += 1, column += 1, all on the device in one launch (eetq_greedy_handover_f16)
void greedy_handover(const Tensor& logits, Tensor& out_tokens, Tensor& column, Tensor& next_token, Tensor& position)
{
    const char* name = "greedy_handover: ";
    TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kHalf && logits.dim() == 2 && logits.stride(1) == 1, name,
                "logits must be a float16 CUDA tensor [B, V] with dense rows");
    const int64_t B = logits.size(0), V = logits.size(1);
    for (const Tensor* t : std::initializer_list<const Tensor*>{&out_tokens, &column, &next_token, &position})
        TORCH_CHECK(t->scalar_type() == at::kLong && t->device() == logits.device(), name, "int64 tensors on the logits' device expected");
    TORCH_CHECK(out_tokens.dim() == 2 && out_tokens.size(0) == B && out_tokens.stride(1) == 1 && next_token.numel() == B &&
                    next_token.is_contiguous() && column.numel() == 1 && position.numel() == 1 && V > 0,
                name, "shape mismatch");
    c10::DeviceGuard guard(logits.device());
    check(eetq_greedy_handover_f16(logits.data_ptr(), (long)logits.stride(0), (int)V, (int)B, out_tokens.data_ptr<int64_t>(),
                                   (long)out_tokens.stride(0), (int)out_tokens.size(1), column.data_ptr<int64_t>(),
                                   next_token.data_ptr<int64_t>(), position.data_ptr<int64_t>(), stream_of(logits)));
}

// Sampling decode hand-over (extension): greedy_handover's bookkeeping with the token drawn by temperature / top-k / top-p sampling
// from a 32-byte device parameter block (int32[8]: eetq_amd.sampling.sampling_params), EOS flags `done` (int32 [B]) and, for
// tests, explicit random numbers `uniforms` (float32 [B]) instead of the kernel's Philox stream (eetq_sample_handover_f16)
void sample_handover(const Tensor& logits, Tensor& out_tokens, Tensor& column, Tensor& next_token, Tensor& position,
                     const Tensor& params, const OptTensor& done, const OptTensor& uniforms)
{
    const char* name = "sample_handover: ";
    TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kHalf && logits.dim() == 2 && logits.stride(1) == 1, name,
                "logits must be a float16 CUDA tensor [B, V] with dense rows");
    const int64_t B = logits.size(0), V = logits.size(1);
    for (const Tensor* t : std::initializer_list<const Tensor*>{&out_tokens, &column, &next_token, &position})
        TORCH_CHECK(t->scalar_type() == at::kLong && t->device() == logits.device(), name, "int64 tensors on the logits' device expected");
    TORCH_CHECK(out_tokens.dim() == 2 && out_tokens.size(0) == B && out_tokens.stride(1) == 1 && next_token.numel() == B &&
                    next_token.is_contiguous() && column.numel() == 1 && position.numel() == 1 && V > 0,
                name, "shape mismatch");
    TORCH_CHECK(params.scalar_type() == at::kInt && params.numel() == 8 && params.is_contiguous() && params.device() == logits.device(),
                name, "params must be a contiguous int32[8] tensor on the logits' device (sampling_params)");
    if (done)
        TORCH_CHECK(done->scalar_type() == at::kInt && done->numel() == B && done->is_contiguous() && done->device() == logits.device(),
                    name, "done must be a contiguous int32 [B] tensor on the logits' device");
    if (uniforms)
        TORCH_CHECK(uniforms->scalar_type() == at::kFloat && uniforms->numel() == B && uniforms->is_contiguous() &&
                        uniforms->device() == logits.device(),
                    name, "uniforms must be a contiguous float32 [B] tensor on the logits' device");
    c10::DeviceGuard guard(logits.device());
    check(eetq_sample_handover_f16(logits.data_ptr(), (long)logits.stride(0), (int)V, (int)B, out_tokens.data_ptr<int64_t>(),
                                   (long)out_tokens.stride(0), (int)out_tokens.size(1), column.data_ptr<int64_t>(),
                                   next_token.data_ptr<int64_t>(), position.data_ptr<int64_t>(), params.data_ptr(),
                                   done ? done->data_ptr<int32_t>() : nullptr, uniforms ? uniforms->data_ptr<float>() : nullptr,
                                   stream_of(logits)));
}

// Prompt-lookup draft of a speculative step (extension): per row of hist [B, cols] (int64, dense rows, any row stride) the k = draft.size(1)
// tokens that followed the longest recent n-gram (n <= max_ngram) repeating the row's tail, L = position + 1 tokens long (a DEVICE
// int64 scalar) -> draft [B, k] (eetq_spec_ngram_draft_i64)
void ngram_draft(const Tensor& hist, const Tensor& position, Tensor& draft, int64_t max_ngram)
{
    const char* name = "ngram_draft: ";
    TORCH_CHECK(hist.is_cuda() && hist.scalar_type() == at::kLong && hist.dim() == 2 && hist.stride(1) == 1 && hist.size(1) > 0, name,
                "hist must be an int64 CUDA tensor [B, cols] with dense rows");
    const int64_t B = hist.size(0);
    for (const Tensor* t : std::initializer_list<const Tensor*>{&position, &draft})
        TORCH_CHECK(t->scalar_type() == at::kLong && t->device() == hist.device(), name, "int64 tensors on the history's device expected");
    TORCH_CHECK(draft.dim() == 2 && draft.size(0) == B && draft.stride(1) == 1 && position.numel() == 1 && B > 0, name, "shape mismatch");
    TORCH_CHECK(draft.size(1) >= 1 && draft.size(1) <= 15, name, "the draft holds 1 .. 15 tokens per row");
    TORCH_CHECK(max_ngram >= 1 && max_ngram <= 8, name, "max_ngram must lie in 1 .. 8");
    c10::DeviceGuard guard(hist.device());
    check(eetq_spec_ngram_draft_i64(hist.data_ptr<int64_t>(), (long)hist.stride(0), (int)hist.size(1), (int)B, position.data_ptr<int64_t>(),
                                    (int)max_ngram, (int)draft.size(1), draft.data_ptr<int64_t>(), (long)draft.stride(0), stream_of(hist)));
}

// Verify, accept and hand-over of a speculative step (extension): logits [B, k + 1, V] (fp16, V dense) of the rows [pending token |
// draft]; the tokens every row confirms go to out_tokens / hist, the last one to next_token; position, column and stats advance on
// the device (eetq_spec_accept_f16)
void spec_accept(const Tensor& logits, const Tensor& draft, Tensor& out_tokens, Tensor& column, Tensor& next_token, Tensor& position,
                 const Tensor& limit, Tensor& hist, Tensor& stats)
{
    const char* name = "spec_accept: ";
    TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kHalf && logits.dim() == 3 && logits.stride(2) == 1, name,
                "logits must be a float16 CUDA tensor [B, k + 1, V] with dense rows");
    const int64_t B = logits.size(0), T = logits.size(1), V = logits.size(2);
    for (const Tensor* t : std::initializer_list<const Tensor*>{&draft, &out_tokens, &column, &next_token, &position, &limit, &hist, &stats})
        TORCH_CHECK(t->scalar_type() == at::kLong && t->device() == logits.device(), name, "int64 tensors on the logits' device expected");
    TORCH_CHECK(T >= 2 && T <= 16 && B > 0 && V > 0 && draft.dim() == 2 && draft.size(0) == B && draft.size(1) == T - 1 &&
                    draft.stride(1) == 1 && out_tokens.dim() == 2 && out_tokens.size(0) == B && out_tokens.stride(1) == 1 &&
                    hist.dim() == 2 && hist.size(0) == B && hist.stride(1) == 1 && next_token.numel() == B &&
                    (next_token.dim() == 1 || (next_token.dim() == 2 && next_token.size(1) == 1)) && column.numel() == 1 &&
                    position.numel() == 1 && limit.numel() == 1 && stats.numel() == 2 && stats.is_contiguous(),
                name, "shape mismatch");
    c10::DeviceGuard guard(logits.device());
    check(eetq_spec_accept_f16(logits.data_ptr(), (long)(B == 1 ? T * V : logits.stride(0)), (long)logits.stride(1), (int)V, (int)B,
                               (int)(T - 1), draft.data_ptr<int64_t>(), (long)draft.stride(0), out_tokens.data_ptr<int64_t>(),
                               (long)out_tokens.stride(0), (int)out_tokens.size(1), column.data_ptr<int64_t>(),
                               position.data_ptr<int64_t>(), limit.data_ptr<int64_t>(), next_token.data_ptr<int64_t>(),
                               (long)(B == 1 ? 1 : next_token.stride(0)), hist.data_ptr<int64_t>(), (long)hist.stride(0),
                               (int)hist.size(1), stats.data_ptr<int64_t>(), stream_of(logits)));
}

// spec_accept for sampled generation (extension): every verify row's token is the one sample_handover draws with `params` at its
// own output column (greedy at temperature 0); a draft token is accepted iff it IS that token; rows finished by `done` (int32 [B])
// or by an EOS token of this step hand on the pad token and never object.  `uniforms`: float32 [B, k + 1] instead of the kernel's
// Philox stream; `workspace`: int64 [B * (k + 1)], allocated here when absent (eager use only) (eetq_spec_sample_accept_f16)
void spec_sample_accept(const Tensor& logits, const Tensor& draft, Tensor& out_tokens, Tensor& column, Tensor& next_token,
                        Tensor& position, const Tensor& limit, Tensor& hist, Tensor& stats, const Tensor& params, const OptTensor& done,
                        const OptTensor& uniforms, const OptTensor& workspace)
{
    const char* name = "spec_sample_accept: ";
    TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kHalf && logits.dim() == 3 && logits.stride(2) == 1, name,
                "logits must be a float16 CUDA tensor [B, k + 1, V] with dense rows");
    const int64_t B = logits.size(0), T = logits.size(1), V = logits.size(2);
    for (const Tensor* t : std::initializer_list<const Tensor*>{&draft, &out_tokens, &column, &next_token, &position, &limit, &hist, &stats})
        TORCH_CHECK(t->scalar_type() == at::kLong && t->device() == logits.device(), name, "int64 tensors on the logits' device expected");
    if (workspace)
        TORCH_CHECK(workspace->scalar_type() == at::kLong && workspace->device() == logits.device(), name,
                    "int64 tensors on the logits' device expected");
    TORCH_CHECK(T >= 2 && T <= 16 && B > 0 && V > 0 && draft.dim() == 2 && draft.size(0) == B && draft.size(1) == T - 1 &&
                    draft.stride(1) == 1 && out_tokens.dim() == 2 && out_tokens.size(0) == B && out_tokens.stride(1) == 1 &&
                    hist.dim() == 2 && hist.size(0) == B && hist.stride(1) == 1 && next_token.numel() == B &&
                    (next_token.dim() == 1 || (next_token.dim() == 2 && next_token.size(1) == 1)) && column.numel() == 1 &&
                    position.numel() == 1 && limit.numel() == 1 && stats.numel() == 2 && stats.is_contiguous(),
                name, "shape mismatch");
    TORCH_CHECK(params.scalar_type() == at::kInt && params.numel() == 8 && params.is_contiguous() && params.device() == logits.device(),
                name, "params must be a contiguous int32[8] tensor on the logits' device (sampling_params)");
    if (done)
        TORCH_CHECK(done->scalar_type() == at::kInt && done->numel() == B && done->is_contiguous() && done->device() == logits.device(),
                    name, "done must be a contiguous int32 [B] tensor on the logits' device");
    if (uniforms)
        TORCH_CHECK(uniforms->scalar_type() == at::kFloat && uniforms->dim() == 2 && uniforms->size(0) == B && uniforms->size(1) == T &&
                        uniforms->stride(1) == 1 && uniforms->device() == logits.device(),
                    name, "uniforms must be a float32 [B, k + 1] tensor with dense rows on the logits' device");
    if (workspace)
        TORCH_CHECK(workspace->numel() >= B * T && workspace->is_contiguous(), name,
                    "workspace must be a contiguous int64 tensor of at least B * (k + 1) elements");
    c10::DeviceGuard guard(logits.device());
    const Tensor ws = workspace ? *workspace : at::empty({B * T}, logits.options().dtype(at::kLong));
    check(eetq_spec_sample_accept_f16(logits.data_ptr(), (long)(B == 1 ? T * V : logits.stride(0)), (long)logits.stride(1), (int)V, (int)B,
                                      (int)(T - 1), draft.data_ptr<int64_t>(), (long)draft.stride(0), out_tokens.data_ptr<int64_t>(),
                                      (long)out_tokens.stride(0), (int)out_tokens.size(1), column.data_ptr<int64_t>(),
                                      position.data_ptr<int64_t>(), limit.data_ptr<int64_t>(), next_token.data_ptr<int64_t>(),
                                      (long)(B == 1 ? 1 : next_token.stride(0)), hist.data_ptr<int64_t>(), (long)hist.stride(0),
                                      (int)hist.size(1), stats.data_ptr<int64_t>(), params.data_ptr(),
                                      done ? done->data_ptr<int32_t>() : nullptr, uniforms ? uniforms->data_ptr<float>() : nullptr,
                                      (long)(!uniforms || B == 1 ? T : uniforms->stride(0)), ws.data_ptr<int64_t>(), stream_of(logits)));
}

Tensor decode_attention(const Tensor& query, const Tensor& key_cache, const Tensor& value_cache, const OptTensor& mask,
                        std::optional<double> scaling, std::optional<int64_t> splits_in, const OptTensor& kv_len,
                        int64_t kv_len_bias, const OptTensor& advance, const OptTensor& kv_start = std::nullopt,
                        std::optional<int64_t> window = std::nullopt, bool ring = false)
{
    if (window) TORCH_CHECK_VALUE(*window >= 1, "decode_attention: window must be at least 1 row (got ", *window, ")");
    check_decode_ring("decode_attention", ring, window, kv_start, mask, kv_len, key_cache.dim() == 4 ? key_cache.size(2) : 0);
    TORCH_CHECK(query.scalar_type() == at::kHalf && key_cache.scalar_type() == at::kHalf && value_cache.scalar_type() == at::kHalf,
                "decode_attention: query and caches must be float16");
    TORCH_CHECK(query.dim() == 3 && key_cache.dim() == 4 && value_cache.sizes() == key_cache.sizes(),
                "decode_attention: expected query [B, H, D] and caches [B, Hkv, S, D]");
    const int64_t B = query.size(0), H = query.size(1), D = query.size(2);
    const int64_t Hkv = key_cache.size(1), S = key_cache.size(2);
    TORCH_CHECK(key_cache.size(0) == B && key_cache.size(3) == D && H % Hkv == 0 && query.stride(-1) == 1 &&
                    key_cache.stride(-1) == 1 && value_cache.stride(-1) == 1,
                "decode_attention: shape / stride mismatch");
    const DecodeAttnPrep p("decode_attention: ", query, S, nullptr, mask, scaling, splits_in, kv_len, advance);
    const auto           strides = p.strides({query.stride(0), query.stride(1)}, key_cache, value_cache);
    const int64_t*       starts  = kv_start_ptr("decode_attention", kv_start, query, B);
    c10::DeviceGuard     guard(query.device());
    if (ring) {   // the windowed entry's bits, the cache rows addressed modulo S
        check(eetq_decode_attention_ring_f16(query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), p.out.data_ptr(),
                                             p.ws.data_ptr<float>(), (int)B, (int)H, (int)Hkv, (int)S, (int)D, (int)p.splits, p.sc,
                                             strides.data(), p.kv_len, (int)kv_len_bias, (int)std::min<int64_t>(*window, INT32_MAX),
                                             p.advance, stream_of(query)));
        return p.out;
    }
    if (window) {   // the last `window` valid rows, not below kv_start (which may be absent)
        check(eetq_decode_attention_window_f16(query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), p.mask(), p.out.data_ptr(),
                                               p.ws.data_ptr<float>(), (int)B, (int)H, (int)Hkv, (int)S, (int)D, (int)p.splits, p.sc,
                                               strides.data(), p.kv_len, (int)kv_len_bias, starts,
                                               (int)std::min<int64_t>(*window, INT32_MAX), p.advance, stream_of(query)));
        return p.out;
    }
    if (starts) {
        check(eetq_decode_attention_padded_f16(query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), p.mask(), p.out.data_ptr(),
                                               p.ws.data_ptr<float>(), (int)B, (int)H, (int)Hkv, (int)S, (int)D, (int)p.splits, p.sc,
                                               strides.data(), p.kv_len, (int)kv_len_bias, starts, p.advance, stream_of(query)));
        return p.out;
    }
    check(eetq_decode_attention_f16(query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), p.mask(), p.out.data_ptr(),
                                    p.ws.data_ptr<float>(), (int)B, (int)H, (int)Hkv, (int)S, (int)D, (int)p.splits, p.sc, strides.data(),
                                    p.kv_len, (int)kv_len_bias, p.advance, stream_of(query)));
    return p.out;
}

// ---- the int8 KV cache (include/eetq_amd.h "The int8 KV cache"): caches int8 [B, Hkv, S, D], scales fp16 [B, Hkv, S, 2] -------------
static void check_i8_cache(const char* name, const Tensor& query, const Tensor& key_cache, const Tensor& value_cache,
                           const Tensor& scales, int64_t B, int64_t Hkv, int64_t D)
{
    TORCH_CHECK(key_cache.scalar_type() == at::kChar && value_cache.scalar_type() == at::kChar && scales.scalar_type() == at::kHalf,
                name, "the caches must be int8 and the scales float16");
    TORCH_CHECK(key_cache.dim() == 4 && value_cache.sizes() == key_cache.sizes() && scales.dim() == 4, name,
                "expected caches [B, Hkv, S, D] and scales [B, Hkv, S, 2]");
    TORCH_CHECK(key_cache.size(0) == B && key_cache.size(1) == Hkv && key_cache.size(3) == D && scales.size(0) == B &&
                    scales.size(1) == Hkv && scales.size(2) == key_cache.size(2) && scales.size(3) == 2,
                name, "shape mismatch");
    TORCH_CHECK(key_cache.stride(-1) == 1 && value_cache.stride(-1) == 1 && scales.stride(-1) == 1, name,
                "cache rows and scale pairs must be dense");
    TORCH_CHECK(key_cache.device() == query.device() && value_cache.device() == query.device() && scales.device() == query.device(),
                name, "all tensors must be on one device");
}

Tensor decode_attention_i8kv(const Tensor& query, const Tensor& key_cache, const Tensor& value_cache, const Tensor& scales,
                             const OptTensor& mask, std::optional<double> scaling, std::optional<int64_t> splits_in,
                             const OptTensor& kv_len, int64_t kv_len_bias, const OptTensor& advance)
{
    const char* name = "decode_attention_i8kv: ";
    TORCH_CHECK(query.scalar_type() == at::kHalf && query.dim() == 3 && query.stride(-1) == 1 && key_cache.dim() == 4, name,
                "expected a float16 query [B, H, D] with dense D");
    const int64_t B = query.size(0), H = query.size(1), D = query.size(2);
    const int64_t Hkv = key_cache.size(1), S = key_cache.size(2);
    check_i8_cache(name, query, key_cache, value_cache, scales, B, Hkv, D);
    TORCH_CHECK(Hkv > 0 && H % Hkv == 0, name, "shape mismatch");
    const DecodeAttnPrep p(name, query, S, nullptr, mask, scaling, splits_in, kv_len, advance);
    const auto           strides = p.strides({query.stride(0), query.stride(1)}, key_cache, value_cache);
    const long           sst[3]  = {(long)scales.stride(0), (long)scales.stride(1), (long)scales.stride(2)};
    c10::DeviceGuard     guard(query.device());
    check(eetq_decode_attention_i8kv_f16(query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), scales.data_ptr(), p.mask(),
                                         p.out.data_ptr(), p.ws.data_ptr<float>(), (int)B, (int)H, (int)Hkv, (int)S, (int)D, (int)p.splits,
                                         p.sc, strides.data(), sst, p.kv_len, (int)kv_len_bias, p.advance, stream_of(query)));
    return p.out;
}

// prefill_attention's device-length / split form over an int8 cache (eetq_prefill_attention_i8kv_f16): query [B, T, H, D] (any token
// / head strides), the first `max_keys` rows of the caches, or clamp(*kv_len + kv_len_bias, 0, max_keys) of them; [B, T, H, D] contiguous
Tensor prefill_attention_i8kv(const Tensor& query, const Tensor& key_cache, const Tensor& value_cache, const Tensor& scales,
                              int64_t max_keys, std::optional<double> scaling, const OptTensor& kv_len, int64_t kv_len_bias,
                              std::optional<int64_t> splits_in, const OptTensor& workspace,
                              std::optional<int64_t> window = std::nullopt, bool ring = false)
{
    const char* name = "prefill_attention_i8kv: ";
    TORCH_CHECK_VALUE(!ring, name, "no ring cache of int8 rows (the ring prompt kernel reads fp16 cache rows only)");
    // accepted only to be refused by name: a caller that passes the fp16 operator's argument must not get the whole prefix silently
    TORCH_CHECK_VALUE(!window, name, "no sliding window on int8 rows (the windowed prompt kernel reads fp16 cache rows only)");
    TORCH_CHECK(query.scalar_type() == at::kHalf && query.is_cuda() && query.dim() == 4 && query.stride(-1) == 1 && key_cache.dim() == 4,
                name, "expected a float16 CUDA query [B, T, H, D] with dense D");
    const int64_t B = query.size(0), T = query.size(1), H = query.size(2), D = query.size(3), Hkv = key_cache.size(1);
    check_i8_cache(name, query, key_cache, value_cache, scales, B, Hkv, D);
    TORCH_CHECK(Hkv > 0 && H % Hkv == 0 && T > 0 && max_keys > 0 && max_keys <= key_cache.size(2), name, "shape mismatch");
    TORCH_CHECK(prefill_attention_supported(D), name, "unsupported head_dim");
    const PromptAttnPrep p(name, query, key_cache, value_cache, max_keys, scaling, kv_len, kv_len_bias, splits_in, workspace,
                           prefill_splits_rule, eetq_prefill_attention_max_splits, eetq_prefill_attention_workspace_floats, false);
    const long sst[3] = {(long)scales.stride(0), (long)scales.stride(1), (long)scales.stride(2)};
    c10::DeviceGuard guard(query.device());
    check(eetq_prefill_attention_i8kv_f16(query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), scales.data_ptr(),
                                          p.out.data_ptr(), p.workspace(), (int)B, (int)H, (int)Hkv, (int)T, (int)max_keys, (int)D, p.kv_len,
                                          (int)kv_len_bias, (int)p.splits, p.sc, p.st, sst, stream_of(query)));
    return p.out;
}

// decode_attention_rows over an int8 cache (eetq_decode_attention_rows_i8kv_f16): query [B, R, H, D] (any row / head strides), R =
// 1 .. 16, the first `max_keys` rows of the caches, or clamp(*kv_len + kv_len_bias, 0, max_keys) of them; [B, R, H, D] contiguous
Tensor decode_attention_rows_i8kv(const Tensor& query, const Tensor& key_cache, const Tensor& value_cache, const Tensor& scales,
                                  int64_t max_keys, std::optional<double> scaling, const OptTensor& kv_len, int64_t kv_len_bias,
                                  std::optional<int64_t> splits_in, const OptTensor& workspace, bool ring = false)
{
    const char* name = "decode_attention_rows_i8kv: ";
    TORCH_CHECK_VALUE(!ring, name, "no ring cache behind the few-row kernel (it reads rows by their logical index)");
    TORCH_CHECK(query.scalar_type() == at::kHalf && query.is_cuda() && query.dim() == 4 && query.stride(-1) == 1 && key_cache.dim() == 4,
                name, "expected a float16 CUDA query [B, R, H, D] with dense D");
    const int64_t B = query.size(0), R = query.size(1), H = query.size(2), D = query.size(3), Hkv = key_cache.size(1);
    check_i8_cache(name, query, key_cache, value_cache, scales, B, Hkv, D);
    TORCH_CHECK(B > 0 && Hkv > 0 && H % Hkv == 0 && max_keys > 0 && max_keys <= key_cache.size(2), name, "shape mismatch");
    TORCH_CHECK(R >= 1 && R <= 16, name, "1 .. 16 query rows per batch row (got ", R, ")");
    TORCH_CHECK(D == 64 || D == 128, name, "unsupported head_dim");
    const PromptAttnPrep p(name, query, key_cache, value_cache, max_keys, scaling, kv_len, kv_len_bias, splits_in, workspace,
                           eetq_decode_attention_rows_splits, eetq_decode_attention_rows_max_splits,
                           eetq_decode_attention_rows_workspace_floats, true);
    const long sst[3] = {(long)scales.stride(0), (long)scales.stride(1), (long)scales.stride(2)};
    c10::DeviceGuard guard(query.device());
    check(eetq_decode_attention_rows_i8kv_f16(query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), scales.data_ptr(),
                                              p.out.data_ptr(), p.workspace(), (int)B, (int)H, (int)Hkv, (int)R, (int)max_keys, (int)D,
                                              p.kv_len, (int)kv_len_bias, (int)p.splits, p.sc, p.st, sst, stream_of(query)));
    return p.out;
}

Tensor rope_decode_attention_i8kv(const Tensor& positions, const Tensor& query, const Tensor& key, const Tensor& value,
                                  const Tensor& cos_sin_cache, Tensor& key_cache, Tensor& value_cache, Tensor& scales,
                                  Tensor& tickets, const OptTensor& slots, const OptTensor& mask, std::optional<double> scaling,
                                  std::optional<int64_t> splits_in, const OptTensor& kv_len, int64_t kv_len_bias,
                                  const OptTensor& advance)
{
    const char* name = "rope_decode_attention_i8kv: ";
    for (const Tensor* t : std::initializer_list<const Tensor*>{&query, &key, &value, &cos_sin_cache})
        TORCH_CHECK(t->scalar_type() == at::kHalf, name, "float16 query, key, value and cos|sin table expected");
    TORCH_CHECK(positions.scalar_type() == at::kLong && positions.is_contiguous(), name, "positions must be contiguous int64");
    TORCH_CHECK(query.dim() == 3 && key.dim() == 3 && value.dim() == 3 && key_cache.dim() == 4, name,
                "expected query [B, H, D], key / value [B, Hkv, D], caches [B, Hkv, S, D]");
    const int64_t B = query.size(0), H = query.size(1), D = query.size(2), Hkv = key.size(1), S = key_cache.size(2);
    check_i8_cache(name, query, key_cache, value_cache, scales, B, Hkv, D);
    TORCH_CHECK(key.size(0) == B && key.size(2) == D && value.sizes() == key.sizes() && Hkv > 0 && H % Hkv == 0 &&
                    positions.numel() == B,
                name, "shape mismatch");
    for (const Tensor* t : std::initializer_list<const Tensor*>{&query, &key, &value})
        TORCH_CHECK(t->stride(-1) == 1 && t->stride(-2) == D, name, "[heads, head_size] must be dense");
    TORCH_CHECK(cos_sin_cache.is_contiguous() && cos_sin_cache.size(-1) == D, name,
                "the rotation must cover the whole head (rot_dim == D)");
    TORCH_CHECK(tickets.scalar_type() == at::kInt && tickets.is_contiguous() && tickets.numel() >= B * H + 1 &&
                    tickets.device() == query.device(),
                name, "tickets must be a zeroed int32 tensor of at least B * H + 1 elements on the device");
    const DecodeAttnPrep p(name, query, S, &slots, mask, scaling, splits_in, kv_len, advance);
    const auto           strides = p.strides({query.stride(0), key.stride(0), value.stride(0)}, key_cache, value_cache);
    const long           sst[3]  = {(long)scales.stride(0), (long)scales.stride(1), (long)scales.stride(2)};
    c10::DeviceGuard     guard(query.device());
    check(eetq_rope_decode_attention_i8kv_f16(
        positions.data_ptr<int64_t>(), p.slots, p.slot_stride, query.data_ptr(), key.data_ptr(), value.data_ptr(),
        cos_sin_cache.data_ptr(), (int)(cos_sin_cache.numel() / D), key_cache.data_ptr(), value_cache.data_ptr(), scales.data_ptr(),
        p.mask(), p.out.data_ptr(), p.ws.data_ptr<float>(), reinterpret_cast<unsigned*>(tickets.data_ptr<int32_t>()), (int)B, (int)H,
        (int)Hkv, (int)S, (int)D, (int)p.splits, p.sc, strides.data(), sst, p.kv_len, (int)kv_len_bias, p.advance, stream_of(query)));
    return p.out;
}

// rotary_embedding_neox_kvcache_prefill writing an int8 cache; key is rotated in place as well
// (eetq_rotary_neox_kvcache_prefill_i8_f16)
void rotary_embedding_neox_kvcache_prefill_i8(const Tensor& positions, Tensor& query, Tensor& key, const Tensor& value,
                                              int64_t head_size, const Tensor& cos_sin_cache, Tensor& key_cache,
                                              Tensor& value_cache, Tensor& scales, int64_t first_row, const OptTensor& first_row_dev)
{
    const char* name = "rotary_embedding_neox_kvcache_prefill_i8: ";
    const auto  p    = rotary_prefill_prep(name, false, positions, query, key, value, head_size, cos_sin_cache, key_cache, value_cache, first_row,
                                           first_row_dev, [&](int64_t B, int64_t Hkv, int64_t D) {
                                           check_i8_cache(name, query, key_cache, value_cache, scales, B, Hkv, D);
                                       });
    const long sst[3] = {(long)scales.stride(0), (long)scales.stride(1), (long)scales.stride(2)};
    c10::DeviceGuard guard(query.device());
    check(eetq_rotary_neox_kvcache_prefill_i8_f16(
        positions.data_ptr<int64_t>(), query.data_ptr(), key.data_ptr(), value.data_ptr(), cos_sin_cache.data_ptr(),
        (int)cos_sin_cache.size(0), key_cache.data_ptr(), value_cache.data_ptr(), scales.data_ptr(), (int)p.B, (int)p.T, p.first_row_dev,
        (int)first_row, (int)p.H, (int)p.Hkv, (int)head_size, (int)cos_sin_cache.size(1), p.strides, sst, (int)key_cache.size(2),
        stream_of(query)));
}

Tensor silu_mul(const Tensor& gate_up, bool glu8)
{
    TORCH_CHECK(gate_up.scalar_type() == at::kHalf && gate_up.is_cuda() && gate_up.is_contiguous(),
                "silu_mul: expected a contiguous float16 CUDA tensor");
    const int64_t inter = gate_up.size(-1) / 2;
    TORCH_CHECK(gate_up.size(-1) == 2 * inter && inter % 8 == 0, "silu_mul: last dimension must be 2*I with I a multiple of 8");
    Tensor        out  = torch::empty(out_shape(gate_up, inter), gate_up.options());
    const int64_t rows = inter ? out.numel() / inter : 0;
    c10::DeviceGuard guard(gate_up.device());
    if (glu8)
        check(eetq_silu_mul_glu8_f16(gate_up.data_ptr(), out.data_ptr(), (int)rows, (int)inter, stream_of(gate_up)));
    else
        check(eetq_silu_mul_f16(gate_up.data_ptr(), out.data_ptr(), (int)rows, (int)inter, stream_of(gate_up)));
    return out;
}

}  // namespace

// One decode step (one new token per batch row) of an accelerated Llama decoder layer over a pre-allocated KV cache, as ONE
// call: the six launches the Python blocks issue (eetq_amd/modules/llama_modules.py: EETLlamaAttention.forward +
// EETLlamaMLP.forward under replace_with_eet_fused_residual), in the same order with the same arguments -- so the result is
// bit-identical -- without ~100 us of interpreter time per layer.  Host-side only; nothing here touches the device directly.
//   qkv  = W8A16(rmsnorm(hidden))                      (norm inside the GEMV launch for a single row)
//   attn = rope_decode_attention(qkv)                  (rotary + cache write + attention, advances `counter`)
//   h    = hidden + W8A16_o(attn)                      (residual in the epilogue)
//   out  = h + W8A16_down(silu(gate) * up),  gate|up = W8A16(rmsnorm(h))
using NormArg = std::tuple<Tensor, double>;
Tensor llama_decode_layer(const Tensor& hidden, const NormArg& input_norm, const Tensor& qkv_w, const Tensor& qkv_s,
                          const OptTensor& qkv_b, const Tensor& positions, const Tensor& cos_sin_cache, Tensor& key_cache,
                          Tensor& value_cache, Tensor& tickets, Tensor& counter, const OptTensor& mask, double scaling,
                          int64_t heads, int64_t kv_heads, const Tensor& o_w, const Tensor& o_s, const OptTensor& o_b,
                          const NormArg& post_norm, const Tensor& gu_w, const Tensor& gu_s, const OptTensor& gu_b,
                          const Tensor& down_w, const Tensor& down_s, const OptTensor& down_b, bool glu8)
{
    TORCH_CHECK(hidden.dim() == 3 && hidden.size(1) == 1, "llama_decode_layer: hidden must be [B, 1, C]");
    const int64_t B = hidden.size(0), total = heads + 2 * kv_heads;
    if (B == 1) {
        // batch 1: straight onto the C ABI -- one device guard, one stream query, one scratch allocation; the same six
        // launches with the same arguments as the generic composition below (bit-identical by construction)
        const int64_t C = hidden.size(2), NQ = qkv_s.numel(), I2 = gu_s.numel(), I = I2 / 2;
        const Tensor &g1 = std::get<0>(input_norm), &g2 = std::get<0>(post_norm);
        TORCH_CHECK(total > 0 && NQ % total == 0, "llama_decode_layer: the QKV width is not (heads + 2 kv_heads) * D");
        const int64_t D = NQ / total, S = key_cache.size(2);
        for (const Tensor* t : std::initializer_list<const Tensor*>{&hidden, &g1, &g2, &qkv_s, &o_s, &gu_s, &down_s, &cos_sin_cache,
                                                                    &key_cache, &value_cache})
            TORCH_CHECK(t->scalar_type() == at::kHalf && t->is_cuda() && t->is_contiguous() && t->device() == hidden.device(),
                        "llama_decode_layer: float16 contiguous tensors on the hidden state's device expected");
        for (const Tensor* t : std::initializer_list<const Tensor*>{&qkv_w, &o_w, &gu_w, &down_w})
            TORCH_CHECK(t->scalar_type() == at::kChar && t->is_contiguous() && t->dim() == 2 && t->device() == hidden.device(),
                        "llama_decode_layer: weights must be contiguous int8 [K, N] on the hidden state's device");
        for (const OptTensor* t : std::initializer_list<const OptTensor*>{&qkv_b, &o_b, &gu_b, &down_b})
            TORCH_CHECK(!*t || ((*t)->scalar_type() == at::kHalf && (*t)->is_contiguous() && (*t)->device() == hidden.device()),
                        "llama_decode_layer: biases must be contiguous float16 on the hidden state's device");
        TORCH_CHECK(qkv_w.size(0) == C && qkv_w.size(1) == NQ && g1.numel() == C && g2.numel() == C && o_w.size(0) == heads * D &&
                        o_w.size(1) == C && o_s.numel() == C && gu_w.size(0) == C && gu_w.size(1) == I2 && I2 == 2 * I &&
                        I % 8 == 0 && down_w.size(0) == I && down_w.size(1) == C && down_s.numel() == C &&
                        (!qkv_b || qkv_b->numel() == NQ) && (!o_b || o_b->numel() == C) && (!gu_b || gu_b->numel() == I2) &&
                        (!down_b || down_b->numel() == C),
                    "llama_decode_layer: weight shapes do not match the hidden size / head geometry");
        TORCH_CHECK(key_cache.dim() == 4 && key_cache.size(0) == 1 && key_cache.size(1) == kv_heads && key_cache.size(3) == D &&
                        value_cache.sizes() == key_cache.sizes() && cos_sin_cache.size(-1) == D && heads % kv_heads == 0,
                    "llama_decode_layer: cache [1, kv_heads, S, D] / rotation table [positions, D] expected");
        TORCH_CHECK(positions.scalar_type() == at::kLong && positions.numel() == 1 && positions.device() == hidden.device() &&
                        counter.scalar_type() == at::kLong && counter.numel() == 1 && counter.device() == hidden.device() &&
                        tickets.scalar_type() == at::kInt && tickets.is_contiguous() && tickets.numel() >= heads + 1 &&
                        tickets.device() == hidden.device(),
                    "llama_decode_layer: positions / counter must be one-element int64, tickets int32 [>= heads + 1], on the device");
        const void* mrow = nullptr;
        if (mask) {
            TORCH_CHECK(mask->scalar_type() == at::kHalf && mask->size(-1) >= S && mask->stride(-1) == 1 &&
                            mask->numel() == mask->size(-1) && mask->device() == hidden.device(),
                        "llama_decode_layer: mask must be one additive float16 row of at least S entries");
            mrow = mask->data_ptr();
        }
        const int64_t splits = eetq_decode_attention_splits(1, (int)heads, (int)S);
        // fp16 scratch: qkv | attention output | gate|up | activation ; fp32 scratch: the attention chunk records
        const int64_t n16 = NQ + heads * D + I2 + I, n32 = heads * splits * (D + 4);
        Tensor  scratch = torch::empty({n16 * 2 + n32 * 4 + 16}, hidden.options().dtype(at::kByte));
        Tensor  h = torch::empty_like(hidden), out = torch::empty_like(hidden);
        char*   base = static_cast<char*>(scratch.data_ptr());
        void *  qkv = base, *att = base + NQ * 2, *gu = base + (NQ + heads * D) * 2, *act = base + (NQ + heads * D + I2) * 2;
        float*  ws  = reinterpret_cast<float*>(base + ((n16 * 2 + 15) / 16) * 16);
        const long st[12] = {(long)NQ, (long)NQ, (long)NQ, (long)key_cache.stride(0), (long)key_cache.stride(1),
                             (long)key_cache.stride(2), (long)value_cache.stride(0), (long)value_cache.stride(1),
                             (long)value_cache.stride(2), 0, (long)(heads * D), (long)D};
        auto optp = [](const OptTensor& t) -> const void* { return t ? t->data_ptr() : nullptr; };
        c10::DeviceGuard guard(hidden.device());
        void*            stream = stream_of(hidden);
        int64_t*         cnt    = counter.data_ptr<int64_t>();
        check(eetq_w8a16_gemv_rmsnorm(hidden.data_ptr(), g1.data_ptr(), (float)std::get<1>(input_norm), qkv_w.data_ptr<int8_t>(),
                                      qkv_s.data_ptr(), optp(qkv_b), nullptr, qkv, (int)NQ, (int)C, stream));
        const char* q = static_cast<const char*>(qkv);
        check(eetq_rope_decode_attention_bounded_f16(positions.data_ptr<int64_t>(), cnt, 0, q, q + heads * D * 2,
                                                     q + (heads + kv_heads) * D * 2, cos_sin_cache.data_ptr(),
                                                     (int)(cos_sin_cache.numel() / D), key_cache.data_ptr(), value_cache.data_ptr(),
                                                     mrow, att, ws, reinterpret_cast<unsigned*>(tickets.data_ptr<int32_t>()), 1,
                                                     (int)heads, (int)kv_heads, (int)S, (int)D, (int)splits, (float)scaling, st, cnt,
                                                     1, cnt, stream));
        check(eetq_w8a16_gemm_act(att, o_w.data_ptr<int8_t>(), o_s.data_ptr(), optp(o_b), hidden.data_ptr(), h.data_ptr(), 1,
                                  (int)C, (int)(heads * D), EETQ_PATH_AUTO, EETQ_ACT_IDENTITY, stream));
        if (glu8) {  // gate|up in "glu8" column order: the activation rides in the projection's epilogue
            check(eetq_w8a16_gemv_glu8(h.data_ptr(), g2.data_ptr(), (float)std::get<1>(post_norm), gu_w.data_ptr<int8_t>(),
                                       gu_s.data_ptr(), optp(gu_b), act, (int)I2, (int)C, stream));
        } else {
            check(eetq_w8a16_gemv_rmsnorm(h.data_ptr(), g2.data_ptr(), (float)std::get<1>(post_norm), gu_w.data_ptr<int8_t>(),
                                          gu_s.data_ptr(), optp(gu_b), nullptr, gu, (int)I2, (int)C, stream));
            check(eetq_silu_mul_f16(gu, act, 1, (int)I, stream));
        }
        check(eetq_w8a16_gemm_act(act, down_w.data_ptr<int8_t>(), down_s.data_ptr(), optp(down_b), h.data_ptr(), out.data_ptr(),
                                  1, (int)C, (int)I, EETQ_PATH_AUTO, EETQ_ACT_IDENTITY, stream));
        return out;
    }
    const std::string autop = "auto", none;
    const std::optional<NormArg> n1(input_norm), n2(post_norm), no_norm;
    const OptTensor no_tensor;
    Tensor qkv = w8_a16_gemm(hidden, qkv_w, qkv_s, autop, qkv_b, no_tensor, n1, false, none);  // [B, 1, (H + 2 Hkv) D]
    TORCH_CHECK(total > 0 && qkv.size(-1) % total == 0, "llama_decode_layer: the QKV width is not (heads + 2 kv_heads) * D");
    const int64_t D = qkv.size(-1) / total;
    Tensor rows = qkv.view({B, total, D});
    Tensor attn = rope_decode_attention(positions, rows.narrow(1, 0, heads), rows.narrow(1, heads, kv_heads),
                                        rows.narrow(1, heads + kv_heads, kv_heads), cos_sin_cache, key_cache, value_cache,
                                        tickets, counter, mask, scaling, std::nullopt, counter, 1, counter);
    Tensor h  = w8_a16_gemm(attn.view({B, 1, heads * D}), o_w, o_s, autop, o_b, hidden, no_norm, false, none);
    Tensor act = glu8 ? w8_a16_gemm(h, gu_w, gu_s, autop, gu_b, no_tensor, n2, false, std::string("silu_glu8"))
                      : silu_mul(w8_a16_gemm(h, gu_w, gu_s, autop, gu_b, no_tensor, n2, false, none));
    return w8_a16_gemm(act, down_w, down_s, autop, down_b, h, no_norm, false, none);
}

// Grouped decode GEMV (extension): independent single-row problems in as few dispatches as possible (eetq_w8a16_gemv_grouped).
// inputs[i]: fp16 with K_i elements (any shape with one row); weights[i]: processed int8 [K_i, N_i]; scales[i]: fp16 [N_i].
// Returns fresh outputs shaped like inputs[i] with the last dimension replaced by N_i.
std::vector<Tensor> w8_a16_gemv_grouped(const std::vector<Tensor>& inputs, const std::vector<Tensor>& weights,
                                        const std::vector<Tensor>& scales, const std::optional<std::vector<OptTensor>>& biases,
                                        const std::optional<std::vector<OptTensor>>& residuals)
{
    const size_t n = inputs.size();
    TORCH_CHECK(weights.size() == n && scales.size() == n, "w8_a16_gemv_grouped: inputs, weights and scales must have one entry per problem");
    TORCH_CHECK(!biases || biases->size() == n, "w8_a16_gemv_grouped: one bias entry (or None) per problem");
    TORCH_CHECK(!residuals || residuals->size() == n, "w8_a16_gemv_grouped: one residual entry (or None) per problem");
    std::vector<Tensor>            outs, keep;
    std::vector<eetq_gemv_problem> probs(n);
    if (n == 0) return outs;
    const auto dev = inputs[0].device();
    for (size_t i = 0; i < n; ++i) {
        const Tensor& x = inputs[i];
        const Tensor& w = weights[i];
        const Tensor& s = scales[i];
        TORCH_CHECK(x.scalar_type() == at::kHalf, "w8_a16_gemm: input must be float16 (got ", x.scalar_type(), ")");
        TORCH_CHECK(x.is_cuda(), "input must be a CUDA tensor");
        TORCH_CHECK(w.scalar_type() == at::kChar && s.scalar_type() == at::kHalf, "w8_a16_gemm: weight must be int8 and scale float16");
        TORCH_CHECK(w.dim() == 2 && w.is_contiguous() && s.is_contiguous(), "w8_a16_gemm: weight [K, N] and scale must be contiguous");
        TORCH_CHECK(x.device() == dev && w.device() == dev && s.device() == dev, "w8_a16_gemv_grouped: all tensors must be on one device");
        const int64_t K = w.size(0), N = w.size(1);
        TORCH_CHECK(x.numel() == K && x.size(-1) == K, "w8_a16_gemv_grouped: every input must be ONE row of K elements");
        TORCH_CHECK(s.numel() == N, "w8_a16_gemm: scale must have N elements");
        Tensor xc = x.is_contiguous() ? x : x.contiguous();
        keep.push_back(xc);
        auto shape = x.sizes().vec();
        shape.back() = N;
        Tensor y = torch::empty(shape, x.options());
        outs.push_back(y);
        probs[i] = eetq_gemv_problem{xc.data_ptr(), w.data_ptr<int8_t>(), s.data_ptr(), y.data_ptr(), nullptr, nullptr, (int)N, (int)K};
        const OptTensor b = biases ? (*biases)[i] : OptTensor();
        const OptTensor r = residuals ? (*residuals)[i] : OptTensor();
        check_epilogue(xc, b, r, 1, N);
        if (b) probs[i].bias = b->data_ptr();
        if (r) probs[i].residual = r->data_ptr();
    }
    c10::DeviceGuard guard(dev);
    check(eetq_w8a16_gemv_grouped(probs.data(), (int)n, stream_of(inputs[0])));
    return outs;
}

// ---- routed mixture-of-experts layers (extensions) ---------------------------------------------------------
// One layer behind every forward below: out[t] = sum_j w[t][j] * down_e( silu(gate_e(x_t)) * up_e(x_t) ), e = top_k_index[t][j], on
// expert stacks gate_up_weight int8 [E, H, 2I] (gfx950 layout per expert, glu8 column order), gate_up_scale fp16 [E, 2I], down_weight
// int8 [E, I, H], down_scale fp16 [E, H].  Ids outside [0, E) contribute nothing.  An entry point is its checks, the source of its
// routing tables (eetq_moe_route on the caller's ids, or the device router) and moe_experts under the plan moe_plan made from the
// shapes; w8_a16_moe_backward is a computation of its own on the same checks.
// The argument checks, each condition stated once (`fn` names the op in the messages, `what` its [T, H] argument) ...
void moe_rows_check(const char* fn, const char* what, const Tensor& x)
{
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kHalf && x.dim() == 2, fn, ": ", what, " must be a float16 GPU tensor [T, H]");
}

struct MoeShape {
    int64_t E, H, N1, I;
};

// ... the expert stacks, on x's device and of x's H.  bits = 4: packed int4 stacks, two values per byte along N --
// gate_up [E, H, I], down [E, I, H / 2] -- and 128-deep tiles; the checks, their order and (for bits = 8) their messages are the same
MoeShape moe_stacks(const char* fn, const char* what, const Tensor& x, const Tensor& gu_w, const Tensor& gu_s, const Tensor& dn_w,
                    const Tensor& dn_s, int bits = 8)
{
    const bool i4 = bits == 4;
    TORCH_CHECK(gu_w.dim() == 3 && dn_w.dim() == 3 && gu_w.scalar_type() == at::kChar && dn_w.scalar_type() == at::kChar &&
                    gu_s.scalar_type() == at::kHalf && dn_s.scalar_type() == at::kHalf,
                fn, i4 ? ": expert weights must be packed int4 stacks (int8 [E, K, N / 2]) and scales float16 [E, N]"
                       : ": expert weights must be int8 [E, K, N] stacks and scales float16 [E, N]");
    const int64_t pack = i4 ? 2 : 1;   // values per byte
    const int64_t E = gu_w.size(0), H = gu_w.size(1), N1 = gu_w.size(2) * pack, I = N1 / 2;
    TORCH_CHECK(N1 == 2 * I && dn_w.size(0) == E && dn_w.size(1) == I && dn_w.size(2) * pack == H && gu_s.dim() == 2 && gu_s.size(0) == E &&
                    gu_s.size(1) == N1 && dn_s.dim() == 2 && dn_s.size(0) == E && dn_s.size(1) == H,
                fn, i4 ? ": expected gate_up_qweight [E, H, I], gate_up_scales [E, 2I], down_qweight [E, I, H / 2], down_scales [E, H]"
                       : ": expected gate_up_weight [E, H, 2I], gate_up_scale [E, 2I], down_weight [E, I, H], down_scale [E, H]");
    if (i4) {
        TORCH_CHECK(H % 128 == 0 && I % 128 == 0, fn, ": the gfx950 int4 layout needs H % 128 == 0 and I % 128 == 0");
    } else {
        TORCH_CHECK(H % 64 == 0 && I % 64 == 0, fn, ": the gfx950 layout needs H % 64 == 0 and I % 64 == 0");
    }
    TORCH_CHECK(gu_w.is_contiguous() && gu_s.is_contiguous() && dn_w.is_contiguous() && dn_s.is_contiguous(),
                fn, ": expert weights and scales must be contiguous");
    for (const Tensor* t : {&gu_w, &gu_s, &dn_w, &dn_s})
        TORCH_CHECK(t->device() == x.device(), fn, ": all tensors must be on the hidden states' device");
    TORCH_CHECK(x.size(1) == H, fn, ": ", what, " is [T, ", x.size(1), "] but the experts have H = ", H);
    return {E, H, N1, I};
}

// ... and the caller's routing
void moe_routing_check(const char* fn, const Tensor& hidden, const Tensor& top_k_index, const Tensor& top_k_weights)
{
    TORCH_CHECK(top_k_index.dim() == 2 && top_k_index.size(0) == hidden.size(0) && top_k_weights.sizes() == top_k_index.sizes(),
                fn, ": top_k_index and top_k_weights must both be [T, k]");
    TORCH_CHECK(top_k_weights.scalar_type() == at::kFloat || top_k_weights.scalar_type() == at::kHalf,
                fn, ": top_k_weights must be float32 or float16");
    TORCH_CHECK(top_k_index.device() == hidden.device() && top_k_weights.device() == hidden.device(),
                fn, ": all tensors must be on the hidden states' device");
}

// EETQ_AMD_MOE_HOST=1 behind EETQ_AMD_TUNING=1 (an A/B hook like every other: the library reads it through tuning_env, once per
// process): T > 16 takes the former host path -- the expert counts read back once, every active expert's rows through the AUTO
// W8A16 GEMMs.  For A/B timing only: it synchronises the stream and cannot be captured.
bool moe_host_path()
{
    static const bool on = eetq_diag_moe_host_path() == 1;
    return on;
}

// Where eetq_w8a16_moe_gemm_tiled takes BOTH projections (its own limits, asked of the library: K >= 320, N K < 2^31 per expert, the
// activation block below 2 GiB): nothing is allocated or expanded for a shape that would then run the decode kernel.
bool moe_i4_tiled_takes(int64_t T, int64_t k, int64_t E, int64_t H, int64_t I)
{
    if (T < 1 || T * k > (int64_t(1) << 30)) return false;
    return eetq_w8a16_moe_gemm_tiled_supported((int)T, (int)k, (int)E, (int)(2 * I), (int)H, 1) == 1 &&
           eetq_w8a16_moe_gemm_tiled_supported((int)T, (int)k, (int)E, (int)H, (int)I, 0) == 1;
}

// Where eetq_w4a16_moe_gemm_tiled takes BOTH projections on the int4 stacks themselves (the limits above with K % 128 == 0 and
// K >= 384 for K = H and K = I)
bool moe_i4_direct_takes(int64_t T, int64_t k, int64_t E, int64_t H, int64_t I)
{
    if (T < 1 || T * k > (int64_t(1) << 30)) return false;
    return eetq_w4a16_moe_gemm_tiled_supported((int)T, (int)k, (int)E, (int)(2 * I), (int)H, 1) == 1 &&
           eetq_w4a16_moe_gemm_tiled_supported((int)T, (int)k, (int)E, (int)H, (int)I, 0) == 1;
}

// What serves one call of the layer: the stacks' format, and for BOTH projections the kernel.
struct MoePlan {
    int  bits;    // 8 or 4
    bool tiled;   // eetq_w8a16_moe_gemm_tiled (128-row LDS tiles, the weight read once per 128 rows); else the decode kernel of `bits`
                  // (16-row MFMA tiles, the expert's weight tile row streamed once per 16 rows)
    bool expand;  // bits = 4 and tiled: eetq_expand_i4_to_i8 of the whole stack in front of each projection
    bool direct;  // bits = 4 and tiled: eetq_w4a16_moe_gemm_tiled on the int4 stack itself -- no expansion, no [E, K, N] buffer
    bool host;    // the A/B host path instead of the grouped kernels
};

// The plan is decided from the SHAPES alone -- the counts live on the device -- so every call with the same (T, k, E, H, I) runs
// the same kernels whatever the routing (a skewed routing costs time, never correctness), and the trainable and the inference
// forward always agree on it.  T <= 16 always takes the decode kernel.
//
// bits = 8: tiled from kMoeTiledMinMeanRows mean rows per expert S / E (a shape outside the tile body's limits still takes the decode
// kernel: moe_project).  The seam is measured (tools/moe_bench.py --seam, profiles/r09_moe_seam.jsonl), one MI355X,
// us per gate|up + down pair of launches, decode kernel / tiled kernel, uniform routing (skewed routing moves no entry across 1.0):
//   mean rows S / E      1        2        4        8        16       32       64
//   qwen3-30b-a3b        87/203   116/211  140/226  161/231  226/229  385/262  662/303
//   mixtral-8x7b         -        -        256/343  301/344  469/406  886/434  1552/519     (4: T = 17, 4.25 rows)
// Below 16 rows per expert the decode kernel wins at both shapes (one 16-row pass streams the weights once; the tiled kernel pays
// 128-row MFMA work and its ring's ramp per tile), at 16 the two meet (Qwen 0.99, Mixtral 1.16 in the tiled kernel's favour),
// above it the decode kernel re-streams the weights once per 16 rows and loses by S / E / 16.
constexpr int64_t kMoeTiledMinMeanRows = 16;

// bits = 4: "decode" is eetq_w4a16_moe_gemm on the int4 tiles, "expand" the expansion of each stack into a torch::empty [E, K, N] int8
// buffer and the tiled kernel on it with the unchanged scales.  The expansion moves 1.5 E K N bytes per projection whatever T is
// (E K N / 2 read, E K N written) and the tiled kernel then reads E_active K N, against ceil(rows / 16) E_active K N / 2 for the
// decode kernel: by bytes alone the two meet near 5 x 16 rows per expert, far above the int8 layer's seam of 16.
// Measured (tools/moe_bench.py --seam --bits 4, profiles/r10_moe_int4_seam.jsonl), one MI355X, us per gate|up + down
// pair, decode kernel / expansions + tiled kernel (of which the two expansions alone: 355 us Mixtral, 157 us Qwen3, whatever T),
// uniform routing (skewed routing moves no entry across 1.0):
//   mean rows S / E      16        32        64         128         256
//   qwen3-30b-a3b        177/369   328/400   583/443    1124/582    2220/787
//   mixtral-8x7b         400/752   708/771   1353/859   2650/1060   5231/1404
// At 32 rows per expert the decode kernel still wins at both shapes (0.82, 0.92), at 64 the expanded path does (1.31, 1.58): the
// seam sits 2-4 x higher than the int8 layer's 16, where the bytes put it.  In rows per expert it is the same at both shapes:
// both sides of the comparison scale with E K N, so E K N drops out of the rule.  (The lines cross near 40 rows by interpolation;
// nothing between 32 and 64 was measured, so the rule starts at the first measured point where the expansion wins.)
constexpr int64_t kMoeI4ExpandMinMeanRows = 64;

// `path` is the int4 ops' argument ("auto" everywhere else): "decode" and "expand" force one side of the int4 rule, "expand" only
// where the tiled kernel takes both projections.  "direct" is the third int4 path: the tiled kernel on the int4 tiles
// (eetq_w4a16_moe_gemm_tiled), bit for bit what "expand" computes without its 1.5 E K N bytes of traffic and its transient stack;
// it raises where that kernel does not take both projections.  "auto" never picks it: its rule stays the measured one above until
// the direct kernel's seam against the decode kernel is measured.  `caller_routed`: the routing is the caller's (w8_a16_moe, w8_a16_moe_train), which
// is where the A/B host switch applies -- never to the block ops, whose tables come from the device router, and never to int4.
MoePlan moe_plan(const char* fn, int bits, const std::string& path, int64_t T, int64_t k, int64_t E, int64_t H, int64_t I,
                 bool caller_routed)
{
    TORCH_CHECK(path == "auto" || path == "decode" || path == "expand" || (bits == 4 && path == "direct"), fn,
                ": path must be 'auto', 'decode' or 'expand', or 'direct'");
    MoePlan p{bits, false, false, false, false};
    if (T == 0) return p;  // nothing runs
    if (bits == 8) {
        p.host  = caller_routed && T > 16 && moe_host_path();
        p.tiled = !p.host && T > 16 && T * k >= kMoeTiledMinMeanRows * E;
        return p;
    }
    TORCH_CHECK(path != "expand" || moe_i4_tiled_takes(T, k, E, H, I),
                fn, ": path='expand' needs a shape the grouped tiled kernel takes (H >= 320 and I >= 320)");
    TORCH_CHECK(path != "direct" || moe_i4_direct_takes(T, k, E, H, I), fn,
                ": path='direct' needs a shape the grouped int4 tiled kernel takes (H and I multiples of 128, both >= 384)");
    p.direct = path == "direct";
    p.expand = path == "expand" ||
               (path == "auto" && T > 16 && T * k >= kMoeI4ExpandMinMeanRows * E && moe_i4_tiled_takes(T, k, E, H, I));
    p.tiled = p.expand || p.direct;
    return p;
}

// 1 where w4_a16_moe(path="direct") runs for these sizes (both projections inside eetq_w4a16_moe_gemm_tiled_supported)
bool w4_a16_moe_direct_supported(int64_t T, int64_t k, int64_t E, int64_t H, int64_t I)
{
    TORCH_CHECK(T >= 0 && k >= 1 && E >= 1 && k <= E && H >= 1 && I >= 1,
                "w4_a16_moe_direct_supported: T >= 0, 1 <= k <= E, H >= 1, I >= 1");
    return E <= (int64_t(1) << 20) && H < (int64_t(1) << 31) && 2 * I < (int64_t(1) << 31) && moe_i4_direct_takes(T, k, E, H, I);
}

std::string w4_a16_moe_path(int64_t T, int64_t k, int64_t E, int64_t H, int64_t I)
{
    TORCH_CHECK(T >= 0 && k >= 1 && E >= 1 && k <= E && H >= 1 && I >= 1, "w4_a16_moe_path: T >= 0, 1 <= k <= E, H >= 1, I >= 1");
    return moe_plan("w4_a16_moe_path", 4, "auto", T, k, E, H, I, true).expand ? "expand" : "decode";
}

// eetq_moe_route's tables in one int32 buffer: counts [E] | offsets [E + 1] | sorted_slot [S] | position [S] | active [A], S = T k
// slots, A = min(E, S)
struct MoeTables {
    int *counts, *offsets, *sorted, *position, *active;
    MoeTables(int* p, int64_t E, int64_t S)
        : counts(p), offsets(p + E), sorted(offsets + E + 1), position(sorted + S), active(position + S)
    {
    }
    static int64_t numel(int64_t E, int64_t S) { return E + (E + 1) + 2 * S + std::min(E, S); }
    static Tensor  alloc(int64_t E, int64_t S, c10::Device dev)
    {
        return torch::empty({numel(E, S)}, at::device(dev).dtype(at::kInt));
    }
};

// What a forward sets up before its first launch (T >= 1): the device guard, the contiguous hidden states, the tables and the view
// of them, the current stream.  It launches nothing.
struct MoeSetup {
    c10::DeviceGuard guard;
    Tensor           hidden, tables;
    MoeTables        t;
    void*            st;
    MoeSetup(const Tensor& hidden_in, const Tensor& tables_in, int64_t E, int64_t S)
        : guard(hidden_in.device()), hidden(hidden_in.contiguous()), tables(tables_in), t(tables.data_ptr<int>(), E, S),
          st(stream_of(hidden_in))
    {
    }
};

// the tables of ids idx [T, k] (int64, contiguous)
void moe_route(const Tensor& idx, int64_t E, const MoeTables& t, void* st)
{
    check(eetq_moe_route(idx.data_ptr<int64_t>(), (int)idx.size(0), (int)idx.size(1), (int)E, t.counts, t.offsets, t.sorted, t.position,
                         t.active, st));
}

// out [T, H] = the router-weighted sum of each token's k rows of y [T k, H] (wts [T, k], float32 or float16)
void moe_combine(const Tensor& y, const int* position, const Tensor& wts, Tensor& out, void* st)
{
    check(eetq_moe_combine_f16(y.data_ptr(), position, wts.data_ptr(), wts.scalar_type() == at::kFloat ? EETQ_DTYPE_F32 : EETQ_DTYPE_F16,
                               out.data_ptr(), (int)out.size(0), (int)wts.size(1), (int)out.size(1), st));
}

// One grouped projection of the layer, y = rows(x) . w [E, K, N] per expert, on the plan's kernel.  An int8 shape outside the tiled
// body's limits (EETQ_ERR_UNSUPPORTED, quiet) takes the decode kernel, which is correct at any row count.  The int4 expansion lives
// for this projection only: at most one expanded stack is alive.
void moe_project(const MoePlan& p, const void* x, const Tensor& w, const Tensor& s, const MoeTables& t, void* y, int64_t T, int64_t k,
                 int64_t E, int64_t N, int64_t K, int gather, int glu8, void* st)
{
    if (p.direct) {  // moe_plan asked eetq_w4a16_moe_gemm_tiled_supported: UNSUPPORTED cannot come back
        check(eetq_w4a16_moe_gemm_tiled(x, w.data_ptr<int8_t>(), s.data_ptr(), t.offsets, t.sorted, t.active, y, (int)T, (int)k, (int)E,
                                        (int)N, (int)K, gather, glu8, /*tile_j*/ 0, st));
        return;
    }
    if (p.tiled) {
        Tensor w8;
        if (p.expand) {
            w8 = torch::empty({E, K, N}, w.options());
            check(eetq_expand_i4_to_i8(w.data_ptr<int8_t>(), w8.data_ptr<int8_t>(), (size_t)w.numel(), st));
        }
        const int rc = eetq_w8a16_moe_gemm_tiled(x, (p.expand ? w8 : w).data_ptr<int8_t>(), s.data_ptr(), t.offsets, t.sorted, t.active, y,
                                                 (int)T, (int)k, (int)E, (int)N, (int)K, gather, glu8, st);
        if (p.expand || rc != EETQ_ERR_UNSUPPORTED) {
            check(rc);
            return;
        }
    }
    check((p.bits == 4 ? eetq_w4a16_moe_gemm : eetq_w8a16_moe_gemm)(x, w.data_ptr<int8_t>(), s.data_ptr(), t.offsets, t.sorted, t.active,
                                                                    y, (int)T, (int)k, (int)E, (int)N, (int)K, gather, glu8, st));
}

// The host path: the expert counts read back once, then every active expert's rows [off, off + c) of the sorted order through the
// dense W8A16 GEMMs into `down`.  Inference (gate_up null): per expert, gate|up with the fused silu_glu8 write-out on the AUTO path,
// then down.  Trainable forward: every expert's gate|up plain into gate_up on the kernel the gated write-out uses (EETQ_PATH_STREAM
// for 2 to 16 rows, AUTO otherwise), one silu_mul over all rows, then every expert's down.
void moe_host_experts(const MoeSetup& c, int64_t k, const Tensor& gu_w, const Tensor& gu_s, const Tensor& dn_w, const Tensor& dn_s,
                      Tensor& down, Tensor* gate_up)
{
    const int64_t E = gu_w.size(0);
    const Tensor  counts_h = c.tables.narrow(0, 0, E).cpu();  // the one host sync of the A/B host path
    const Tensor  sorted_t = c.tables.narrow(0, c.t.sorted - c.t.counts, c.hidden.size(0) * k);
    std::vector<std::tuple<int64_t, int64_t, int64_t>> experts;  // e, off, c
    int64_t                                            n = 0;
    for (int64_t e = 0; e < E; ++e)
        if (const int64_t cnt = counts_h.data_ptr<int>()[e]) {
            experts.emplace_back(e, n, cnt);
            n += cnt;
        }
    auto gathered = [&](int64_t off, int64_t cnt) { return c.hidden.index_select(0, sorted_t.narrow(0, off, cnt).div(k, "floor")); };
    auto project  = [](const Tensor& in, const Tensor& w, const Tensor& s, Tensor& y, int64_t off, int64_t cnt, int path) {
        Tensor rows = y.narrow(0, off, cnt);
        gemm_launch(in, w, s, rows, cnt, s.numel(), in.size(1), path, std::nullopt, std::nullopt, EETQ_ACT_IDENTITY);
    };
    for (const auto& [e, off, cnt] : experts) {
        if (gate_up) {
            project(gathered(off, cnt), gu_w[e], gu_s[e], *gate_up, off, cnt, cnt >= 2 && cnt <= 16 ? EETQ_PATH_STREAM : EETQ_PATH_AUTO);
            continue;
        }
        const Tensor gate = w8_a16_gemm(gathered(off, cnt), gu_w[e], gu_s[e], "auto", std::nullopt, std::nullopt, std::nullopt, false,
                                        std::string("silu_glu8"));
        project(gate, dn_w[e], dn_s[e], down, off, cnt, EETQ_PATH_AUTO);
    }
    if (!gate_up || !n) return;
    const Tensor inter = silu_mul(gate_up->narrow(0, 0, n), true);
    for (const auto& [e, off, cnt] : experts) project(inter.narrow(0, off, cnt), dn_w[e], dn_s[e], down, off, cnt, EETQ_PATH_AUTO);
}

// The experts on routed rows (the tables of c are filled, or their launch is queued on c.st): grouped GEMM (gather) -> grouped GEMM
// (sorted rows) -> combine with wts [T, k] into out [T, H]; no host sync, capturable.  Inference (gate_up null): the first GEMM writes
// silu(gate) * up itself (glu8 = 1), three launches.  Trainable forward: it writes the plain gate|up projection into gate_up [T k, 2I]
// and eetq_silu_mul_glu8_f16 follows, four launches -- the glu8 write-out of either grouped kernel is the plain projection followed
// by that launch bit for bit.  y [T k, H], when given, receives each sorted row's down projection.
void moe_experts(const MoePlan& p, const MoeSetup& c, const Tensor& wts, const MoeShape& m, const Tensor& gu_w, const Tensor& gu_s,
                 const Tensor& dn_w, const Tensor& dn_s, Tensor& out, Tensor* gate_up = nullptr, Tensor* y = nullptr)
{
    const int64_t T = c.hidden.size(0), k = wts.size(1), S = T * k;
    Tensor        down = y ? *y : torch::empty({S, m.H}, c.hidden.options());
    if (p.host) {
        moe_host_experts(c, k, gu_w, gu_s, dn_w, dn_s, down, gate_up);
    } else {
        Tensor inter = torch::empty({S, m.I}, c.hidden.options());
        moe_project(p, c.hidden.data_ptr(), gu_w, gu_s, c.t, gate_up ? gate_up->data_ptr() : inter.data_ptr(), T, k, m.E, m.N1, m.H, 1,
                    gate_up ? 0 : 1, c.st);
        if (gate_up) check(eetq_silu_mul_glu8_f16(gate_up->data_ptr(), inter.data_ptr(), (int)S, (int)m.I, c.st));
        moe_project(p, inter.data_ptr(), dn_w, dn_s, c.t, down.data_ptr(), T, k, m.E, m.H, m.I, 0, 0, c.st);
    }
    moe_combine(down, c.t.position, wts, out, c.st);
}

// The three layer ops: the caller's routing, eetq_moe_route in front of the experts (four launches at inference, five for the
// trainable forward, any T).  `keep`: the trainable forward's outputs next to `out` -- the routing tables (int32, counts | offsets |
// sorted_slot | position | active), gate_up [T*k, 2I] (the gate|up projection of every sorted row, glu8 column order, before the
// activation) and y [T*k, H] (each sorted row's down projection, before the router weighting); rows past offsets[E] of both are
// unspecified.
using MoeLayerOut = std::tuple<Tensor, Tensor, Tensor, Tensor>;  // out, tables, gate_up, y

MoeLayerOut moe_layer(const char* fn, int bits, const std::string& path, bool keep, const Tensor& hidden_in, const Tensor& top_k_index,
                      const Tensor& top_k_weights, const Tensor& gu_w, const Tensor& gu_s, const Tensor& dn_w, const Tensor& dn_s)
{
    moe_rows_check(fn, "hidden", hidden_in);
    const MoeShape m = moe_stacks(fn, "hidden", hidden_in, gu_w, gu_s, dn_w, dn_s, bits);
    moe_routing_check(fn, hidden_in, top_k_index, top_k_weights);
    const int64_t T = hidden_in.size(0), k = top_k_index.size(1), S = T * k;
    const MoePlan p = moe_plan(fn, bits, path, T, k, m.E, m.H, m.I, true);
    Tensor        out    = torch::empty({T, m.H}, hidden_in.options());
    Tensor        tables = MoeTables::alloc(m.E, S, hidden_in.device());
    Tensor        gate_up, y;
    if (keep) {
        gate_up = torch::empty({S, m.N1}, hidden_in.options());
        y       = torch::empty({S, m.H}, hidden_in.options());
    }
    if (T == 0) return {out, tables, gate_up, y};
    const MoeSetup c(hidden_in, tables, m.E, S);
    const Tensor   idx = top_k_index.to(at::kLong).contiguous(), wts = top_k_weights.contiguous();
    moe_route(idx, m.E, c.t, c.st);
    moe_experts(p, c, wts, m, gu_w, gu_s, dn_w, dn_s, out, keep ? &gate_up : nullptr, keep ? &y : nullptr);
    return {out, tables, gate_up, y};
}

// Routed W8A16 mixture-of-experts layer: the forward of transformers' experts modules.
Tensor w8_a16_moe(const Tensor& hidden, const Tensor& top_k_index, const Tensor& top_k_weights, const Tensor& gu_w, const Tensor& gu_s,
                  const Tensor& dn_w, const Tensor& dn_s)
{
    return std::get<0>(moe_layer("w8_a16_moe", 8, "auto", false, hidden, top_k_index, top_k_weights, gu_w, gu_s, dn_w, dn_s));
}

// Trainable forward of the layer: the same `out` as w8_a16_moe bit for bit -- the plan is the same -- plus what the
// backward reads.  (Under the A/B host switch: w8_a16_moe's host path with each expert's gate|up run plain on the kernel its gated
// write-out uses, then one silu_mul over all rows.)
std::tuple<Tensor, Tensor, Tensor, Tensor> w8_a16_moe_train(const Tensor& hidden, const Tensor& top_k_index, const Tensor& top_k_weights,
                                                            const Tensor& gu_w, const Tensor& gu_s, const Tensor& dn_w, const Tensor& dn_s)
{
    return moe_layer("w8_a16_moe_train", 8, "auto", true, hidden, top_k_index, top_k_weights, gu_w, gu_s, dn_w, dn_s);
}

// Routed W4A16 mixture-of-experts layer: w8_a16_moe on int4 expert stacks -- gate_up_qweight int8 [E, H, I]
// (= [E, K = H, N / 2], N = 2I: two values per byte; per expert the gfx950 int4 layout, glu8 column order), gate_up_scales fp16
// [E, 2I], down_qweight int8 [E, I, H / 2], down_scales fp16 [E, H].  This op is the inference forward (w4_a16_moe_train /
// w4_a16_moe_backward below train through the layer); eetq_moe_route and eetq_moe_combine_f16 are the int8 layer's, unchanged.
// w4_a16_moe_path reports what path = "auto" runs.
Tensor w4_a16_moe(const Tensor& hidden, const Tensor& top_k_index, const Tensor& top_k_weights, const Tensor& gu_w, const Tensor& gu_s,
                  const Tensor& dn_w, const Tensor& dn_s, const std::string& path)
{
    return std::get<0>(moe_layer("w4_a16_moe", 4, path, false, hidden, top_k_index, top_k_weights, gu_w, gu_s, dn_w, dn_s));
}

// Backward of w8_a16_moe_train with the int8 weights frozen (extension): the gradients of the hidden states
// (need_input_grad) and of top_k_weights (need_weights_grad, in their dtype), None where not asked for.  Five launches for any T,
// no host sync (capturable), deterministic:
//   eetq_moe_combine_bwd_f16 (dy = dout * w per sorted row, dw) -> eetq_w8a16_moe_gemm_t over the down stack (dh) ->
//   eetq_silu_mul_glu8_bwd_f16 (dgate_up, glu8 order) -> eetq_w8a16_moe_gemm_t over the gate|up stack (per-slot dx) ->
//   eetq_moe_combine_f16 with unit weights (the sum over each token's slots in j order).
// The saved tensors are only read, so a retained graph can run it again.
// bits = 4 (w4_a16_moe_backward): the same five launches on int4 stacks, eetq_w4a16_moe_gemm_t reading the int4 tiles
// for the two transposed GEMMs -- no stack is expanded, the extra memory is the same activations.  `fn` names the op and `train` its
// forward in the messages.
std::tuple<OptTensor, OptTensor> moe_backward(const char* fn, const char* train, int bits, const Tensor& grad_out,
                                              const Tensor& top_k_weights, const Tensor& tables, const Tensor& gate_up, const Tensor& y,
                                              const Tensor& gu_w, const Tensor& gu_s, const Tensor& dn_w, const Tensor& dn_s,
                                              bool need_input_grad, bool need_weights_grad)
{
    moe_rows_check(fn, "grad_out", grad_out);
    const auto [E, H, N1, I] = moe_stacks(fn, "grad_out", grad_out, gu_w, gu_s, dn_w, dn_s, bits);
    const auto gemm_t        = bits == 4 ? eetq_w4a16_moe_gemm_t : eetq_w8a16_moe_gemm_t;
    TORCH_CHECK(top_k_weights.dim() == 2 && top_k_weights.size(0) == grad_out.size(0) && top_k_weights.device() == grad_out.device() &&
                    (top_k_weights.scalar_type() == at::kFloat || top_k_weights.scalar_type() == at::kHalf),
                fn, ": top_k_weights must be float32 or float16 [T, k] on grad_out's device");
    const int64_t T = grad_out.size(0), k = top_k_weights.size(1), S = T * k;
    TORCH_CHECK(tables.is_cuda() && tables.scalar_type() == at::kInt && tables.is_contiguous() && tables.dim() == 1 &&
                    tables.numel() == MoeTables::numel(E, S) && tables.device() == grad_out.device(),
                fn, ": tables must be ", train, "'s int32 routing tables for these T, k and E");
    TORCH_CHECK(gate_up.scalar_type() == at::kHalf && gate_up.is_contiguous() && gate_up.dim() == 2 && gate_up.size(0) == S &&
                    gate_up.size(1) == N1 && gate_up.device() == grad_out.device(),
                fn, ": gate_up must be ", train, "'s contiguous float16 [T*k, 2I]");
    TORCH_CHECK(y.scalar_type() == at::kHalf && y.is_contiguous() && y.dim() == 2 && y.size(0) == S && y.size(1) == H &&
                    y.device() == grad_out.device(),
                fn, ": y must be ", train, "'s contiguous float16 [T*k, H]");
    OptTensor gx, gw;
    if (!need_input_grad && !need_weights_grad) return {gx, gw};
    const Tensor wts = top_k_weights.contiguous();
    if (T == 0) {
        if (need_input_grad) gx = torch::empty({0, H}, grad_out.options());
        if (need_weights_grad) gw = torch::empty_like(wts);
        return {gx, gw};
    }
    c10::DeviceGuard guard(grad_out.device());
    void*      st   = stream_of(grad_out);
    Tensor     dout = grad_out.contiguous();  // a stride-0 gradient (out.sum().backward()) is materialised here
    if (reinterpret_cast<uintptr_t>(dout.data_ptr()) % 16 != 0) dout = dout.clone();
    const MoeTables t(tables.data_ptr<int>(), E, S);
    const int       wdt = wts.scalar_type() == at::kFloat ? EETQ_DTYPE_F32 : EETQ_DTYPE_F16;
    Tensor          dy  = torch::empty({S, H}, grad_out.options());
    if (need_weights_grad) gw = torch::empty_like(wts);
    check(eetq_moe_combine_bwd_f16(dout.data_ptr(), y.data_ptr(), t.position, wts.data_ptr(), wdt, dy.data_ptr(),
                                   need_weights_grad ? gw->data_ptr() : nullptr, (int)T, (int)k, (int)H, st));
    if (!need_input_grad) return {gx, gw};
    // each temporary is released as soon as the next step has consumed it: the peak is dh + dgate_up (+ dy, dx per slot)
    Tensor dh = torch::empty({S, I}, grad_out.options());
    check(gemm_t(dy.data_ptr(), dn_w.data_ptr<int8_t>(), dn_s.data_ptr(), t.offsets, t.active, dh.data_ptr(), (int)T, (int)k, (int)E,
                 (int)H, (int)I, st));
    dy.reset();
    Tensor dgu = torch::empty({S, N1}, grad_out.options());
    check(eetq_silu_mul_glu8_bwd_f16(gate_up.data_ptr(), dh.data_ptr(), dgu.data_ptr(), (int)S, (int)I, st));
    dh.reset();
    Tensor dxs = torch::empty({S, H}, grad_out.options());
    check(gemm_t(dgu.data_ptr(), gu_w.data_ptr<int8_t>(), gu_s.data_ptr(), t.offsets, t.active, dxs.data_ptr(), (int)T, (int)k, (int)E,
                 (int)N1, (int)H, st));
    dgu.reset();
    const Tensor ones = torch::ones({T, k}, grad_out.options().dtype(at::kFloat));
    gx                = torch::empty({T, H}, grad_out.options());
    moe_combine(dxs, t.position, ones, *gx, st);
    return {gx, gw};
}

std::tuple<OptTensor, OptTensor> w8_a16_moe_backward(const Tensor& grad_out, const Tensor& top_k_weights, const Tensor& tables,
                                                     const Tensor& gate_up, const Tensor& y, const Tensor& gu_w, const Tensor& gu_s,
                                                     const Tensor& dn_w, const Tensor& dn_s, bool need_input_grad,
                                                     bool need_weights_grad)
{
    return moe_backward("w8_a16_moe_backward", "w8_a16_moe_train", 8, grad_out, top_k_weights, tables, gate_up, y, gu_w, gu_s, dn_w,
                        dn_s, need_input_grad, need_weights_grad);
}

// Trainable forward and backward of the W4A16 layer: w8_a16_moe_train / w8_a16_moe_backward on int4 stacks.  The
// forward runs w4_a16_moe's plan for the same `path`, so `out` is w4_a16_moe's bit for bit on every path.
MoeLayerOut w4_a16_moe_train(const Tensor& hidden, const Tensor& top_k_index, const Tensor& top_k_weights, const Tensor& gu_w,
                             const Tensor& gu_s, const Tensor& dn_w, const Tensor& dn_s, const std::string& path)
{
    return moe_layer("w4_a16_moe_train", 4, path, true, hidden, top_k_index, top_k_weights, gu_w, gu_s, dn_w, dn_s);
}

std::tuple<OptTensor, OptTensor> w4_a16_moe_backward(const Tensor& grad_out, const Tensor& top_k_weights, const Tensor& tables,
                                                     const Tensor& gate_up, const Tensor& y, const Tensor& gu_w, const Tensor& gu_s,
                                                     const Tensor& dn_w, const Tensor& dn_s, bool need_input_grad,
                                                     bool need_weights_grad)
{
    return moe_backward("w4_a16_moe_backward", "w4_a16_moe_train", 4, grad_out, top_k_weights, tables, gate_up, y, gu_w, gu_s, dn_w,
                        dn_s, need_input_grad, need_weights_grad);
}

// ---- the MoE router on the device (extension) ----------------------------------------------------------------
// What transformers' *TopKRouter forwards return -- (router_logits fp16 [T, E], router_scores [T, k], router_indices int64 [T, k])
// -- from hidden [T, H] and the router weight [E, H].  T <= 16: eetq_moe_router_f16, ONE launch, which also fills `t` (when given)
// with eetq_moe_route's tables for its indices.  T > 16: the logits are a real GEMM and stay at::linear's; eetq_moe_topk_f16 and
// (with `t`) eetq_moe_route follow: three launches.  No host sync either way.
struct RouterOut {
    Tensor logits, scores, idx;
};

// The routing rule.  bias undefined: the softmax rule above (fp16 logits).  bias defined: the sigmoid, bias-corrected, group-limited
// rule of DeepseekV3TopkRouter -- fp32 logits, fp32 weights = sigmoid (renormalised) * scale -- on
// eetq_moe_router_sigmoid_f16 (T <= 16, one launch) or at::linear in fp32, eetq_moe_topk_sigmoid_f32 and eetq_moe_route above it.
struct RouterRule {
    Tensor  bias;  // e_score_correction_bias [E], fp16 or fp32
    int64_t n_group = 1, topk_group = 1;
    double  scale = 1.0;
    bool    sigmoid() const { return bias.defined(); }
    int     bias_dtype() const { return bias.scalar_type() == at::kFloat ? EETQ_DTYPE_F32 : EETQ_DTYPE_F16; }
};

at::ScalarType router_scores_dtype(const char* fn, const py::object& scores_dtype)
{
    const at::ScalarType dt = scores_dtype.is_none() ? at::kFloat : torch::python::detail::py_object_to_dtype(scores_dtype);
    TORCH_CHECK(dt == at::kFloat || dt == at::kHalf, fn, ": scores_dtype must be torch.float32 or torch.float16");
    return dt;
}

void router_check(const char* fn, const Tensor& hidden, const Tensor& weight, int64_t top_k)
{
    moe_rows_check(fn, "hidden", hidden);
    TORCH_CHECK(weight.scalar_type() == at::kHalf && weight.dim() == 2 && weight.device() == hidden.device(),
                fn, ": the router weight must be a float16 tensor [E, H] on the hidden states' device");
    TORCH_CHECK(weight.size(1) == hidden.size(1), fn, ": hidden is [T, ", hidden.size(1), "] but the router weight has H = ", weight.size(1));
    TORCH_CHECK(top_k >= 1 && top_k <= weight.size(0), fn, ": top_k must be in [1, E]");
    TORCH_CHECK(hidden.size(0) * weight.size(0) < (1ll << 31) && hidden.size(0) * top_k <= (1ll << 30), fn, ": too many tokens");
}

// the sigmoid rule's arguments against the router weight [E, H] (the C entries check the same limits; here before any launch)
RouterRule router_rule(const char* fn, const Tensor& weight, const Tensor& bias, int64_t top_k, int64_t n_group, int64_t topk_group,
                       double scale)
{
    const int64_t E = weight.size(0);
    TORCH_CHECK(bias.defined() && bias.dim() == 1 && bias.size(0) == E && bias.device() == weight.device() &&
                    (bias.scalar_type() == at::kHalf || bias.scalar_type() == at::kFloat),
                fn, ": the correction bias must be a float16 or float32 tensor [E] on the router weight's device");
    TORCH_CHECK(n_group >= 1 && n_group <= 64 && E % n_group == 0 && (n_group == 1 || E / n_group >= 2), fn,
                ": n_group must be in [1, 64] and divide E into groups of at least two experts (E = ", E, ", n_group = ", n_group, ")");
    TORCH_CHECK(topk_group >= 1 && topk_group <= n_group, fn, ": topk_group must be in [1, n_group]");
    TORCH_CHECK(top_k <= topk_group * (E / n_group), fn, ": top_k exceeds the experts of the topk_group kept groups");
    TORCH_CHECK(std::isfinite(scale), fn, ": routed_scaling_factor must be finite");
    RouterRule r;
    r.bias       = bias.detach().contiguous();
    r.n_group    = n_group;
    r.topk_group = topk_group;
    r.scale      = scale;
    return r;
}

// hidden and weight contiguous, T >= 1, the device guard set by the caller
RouterOut router_launch(const Tensor& hidden, const Tensor& weight, const RouterRule& rule, int64_t k, bool renorm, at::ScalarType sdt,
                        const MoeTables* t, void* st)
{
    const int64_t T = hidden.size(0), H = hidden.size(1), E = weight.size(0);
    const int     wdt = sdt == at::kFloat ? EETQ_DTYPE_F32 : EETQ_DTYPE_F16;
    const bool    sig = rule.sigmoid();
    RouterOut     r;
    r.scores = torch::empty({T, k}, hidden.options().dtype(sdt));
    r.idx    = torch::empty({T, k}, hidden.options().dtype(at::kLong));
    if (T <= 16) {
        r.logits = torch::empty({T, E}, hidden.options().dtype(sig ? at::kFloat : at::kHalf));
        int* const tb[5] = {t ? t->counts : nullptr, t ? t->offsets : nullptr, t ? t->sorted : nullptr, t ? t->position : nullptr,
                            t ? t->active : nullptr};
        if (sig)
            check(eetq_moe_router_sigmoid_f16(hidden.data_ptr(), weight.data_ptr(), rule.bias.data_ptr(), rule.bias_dtype(), (int)T, (int)H,
                                              (int)E, (int)k, (int)rule.n_group, (int)rule.topk_group, renorm ? 1 : 0, (float)rule.scale,
                                              wdt, r.logits.data_ptr(), r.idx.data_ptr<int64_t>(), r.scores.data_ptr(), tb[0], tb[1],
                                              tb[2], tb[3], tb[4], st));
        else
            check(eetq_moe_router_f16(hidden.data_ptr(), weight.data_ptr(), (int)T, (int)H, (int)E, (int)k, renorm ? 1 : 0, wdt,
                                      r.logits.data_ptr(), r.idx.data_ptr<int64_t>(), r.scores.data_ptr(), tb[0], tb[1], tb[2], tb[3],
                                      tb[4], st));
        return r;
    }
    {
        at::NoGradGuard no_grad;
        r.logits = (sig ? at::linear(hidden.to(at::kFloat), weight.to(at::kFloat)) : at::linear(hidden, weight)).contiguous();
    }
    if (sig)
        check(eetq_moe_topk_sigmoid_f32(r.logits.data_ptr(), rule.bias.data_ptr(), rule.bias_dtype(), (int)T, (int)E, (int)k,
                                        (int)rule.n_group, (int)rule.topk_group, renorm ? 1 : 0, (float)rule.scale, wdt,
                                        r.idx.data_ptr<int64_t>(), r.scores.data_ptr(), st));
    else
        check(eetq_moe_topk_f16(r.logits.data_ptr(), (int)T, (int)E, (int)k, renorm ? 1 : 0, wdt, r.idx.data_ptr<int64_t>(),
                                r.scores.data_ptr(), st));
    if (t) moe_route(r.idx, E, *t, st);
    return r;
}

// the router op of either rule: (logits, scores, idx)
RouterOut router_op(const Tensor& hidden_in, const Tensor& weight_in, const RouterRule& rule, int64_t top_k, bool renorm,
                    at::ScalarType sdt)
{
    const int64_t T = hidden_in.size(0), E = weight_in.size(0);
    if (T == 0)
        return {torch::empty({0, E}, hidden_in.options().dtype(rule.sigmoid() ? at::kFloat : at::kHalf)),
                torch::empty({0, top_k}, hidden_in.options().dtype(sdt)), torch::empty({0, top_k}, hidden_in.options().dtype(at::kLong))};
    c10::DeviceGuard guard(hidden_in.device());
    const Tensor     hidden = hidden_in.detach().contiguous(), weight = weight_in.detach().contiguous();
    return router_launch(hidden, weight, rule, top_k, renorm, sdt, nullptr, stream_of(hidden_in));
}

std::tuple<Tensor, Tensor, Tensor> moe_router(const Tensor& hidden_in, const Tensor& weight_in, int64_t top_k, bool norm_topk_prob,
                                              const py::object& scores_dtype)
{
    const at::ScalarType sdt = router_scores_dtype("moe_router", scores_dtype);
    router_check("moe_router", hidden_in, weight_in, top_k);
    const RouterOut r = router_op(hidden_in, weight_in, RouterRule{}, top_k, norm_topk_prob, sdt);
    return {r.logits, r.scores, r.idx};
}

// DeepseekV3TopkRouter.forward on the device (extension): the reference's triple in the reference's order --
// (router_logits fp32 [T, E], top_k_weights fp32 [T, k], top_k_index int64 [T, k]).
std::tuple<Tensor, Tensor, Tensor> moe_router_sigmoid(const Tensor& hidden_in, const Tensor& weight_in, const Tensor& bias, int64_t top_k,
                                                      int64_t n_group, int64_t topk_group, bool norm_topk_prob,
                                                      double routed_scaling_factor)
{
    router_check("moe_router_sigmoid", hidden_in, weight_in, top_k);
    const RouterRule rule = router_rule("moe_router_sigmoid", weight_in, bias, top_k, n_group, topk_group, routed_scaling_factor);
    const RouterOut  r    = router_op(hidden_in, weight_in, rule, top_k, norm_topk_prob, at::kFloat);
    return {r.logits, r.scores, r.idx};
}

// The whole sparse MoE block (extension): router -> moe_experts on the stacks of w8_a16_moe (bits = 8) or w4_a16_moe
// (bits = 4).  The same launches as those layers on the router's output, bit for bit; only the tables come from the router launch
// (T <= 16: four launches in all) instead of a launch of their own.
// `bias` defined: the sigmoid rule (fp32 weights; scores_dtype is not read), else the softmax rule.
Tensor moe_block(const char* fn, int bits, const Tensor& hidden_in, const Tensor& router_w, const Tensor& bias, int64_t n_group,
                 int64_t topk_group, double scale, int64_t top_k, bool norm_topk_prob, const py::object& scores_dtype, const Tensor& gu_w,
                 const Tensor& gu_s, const Tensor& dn_w, const Tensor& dn_s, const std::string& path)
{
    const at::ScalarType sdt = bias.defined() ? at::kFloat : router_scores_dtype(fn, scores_dtype);
    router_check(fn, hidden_in, router_w, top_k);
    const RouterRule rule = bias.defined() ? router_rule(fn, router_w, bias, top_k, n_group, topk_group, scale) : RouterRule{};
    const MoeShape m = moe_stacks(fn, "hidden", hidden_in, gu_w, gu_s, dn_w, dn_s, bits);
    TORCH_CHECK(router_w.size(0) == m.E, fn, ": the router weight has ", router_w.size(0), " experts but the stacks have E = ", m.E);
    const int64_t T = hidden_in.size(0), S = T * top_k;
    const MoePlan p = moe_plan(fn, bits, path, T, top_k, m.E, m.H, m.I, false);
    Tensor        out = torch::empty({T, m.H}, hidden_in.options());
    if (T == 0) return out;
    const MoeSetup  c(hidden_in.detach(), MoeTables::alloc(m.E, S, hidden_in.device()), m.E, S);
    const Tensor    weight = router_w.detach().contiguous();
    const RouterOut r = router_launch(c.hidden, weight, rule, top_k, norm_topk_prob, sdt, &c.t, c.st);
    moe_experts(p, c, r.scores, m, gu_w, gu_s, dn_w, dn_s, out);
    return out;
}

Tensor w8_a16_moe_block(const Tensor& hidden, const Tensor& router_weight, int64_t top_k, bool norm_topk_prob, const py::object& scores_dtype,
                        const Tensor& gu_w, const Tensor& gu_s, const Tensor& dn_w, const Tensor& dn_s)
{
    return moe_block("w8_a16_moe_block", 8, hidden, router_weight, Tensor(), 1, 1, 1.0, top_k, norm_topk_prob, scores_dtype, gu_w, gu_s,
                     dn_w, dn_s, "auto");
}

Tensor w4_a16_moe_block(const Tensor& hidden, const Tensor& router_weight, int64_t top_k, bool norm_topk_prob, const py::object& scores_dtype,
                        const Tensor& gu_w, const Tensor& gu_s, const Tensor& dn_w, const Tensor& dn_s, const std::string& path)
{
    return moe_block("w4_a16_moe_block", 4, hidden, router_weight, Tensor(), 1, 1, 1.0, top_k, norm_topk_prob, scores_dtype, gu_w, gu_s,
                     dn_w, dn_s, path);
}

// The DeepSeek-V3 family's routed half of the block: the sigmoid router in front of the same experts; the shared
// expert stays the caller's.
Tensor w8_a16_moe_block_sigmoid(const Tensor& hidden, const Tensor& router_weight, const Tensor& bias, int64_t top_k, int64_t n_group,
                                int64_t topk_group, bool norm_topk_prob, double routed_scaling_factor, const Tensor& gu_w,
                                const Tensor& gu_s, const Tensor& dn_w, const Tensor& dn_s)
{
    TORCH_CHECK(bias.defined(), "w8_a16_moe_block_sigmoid: the correction bias is required");
    return moe_block("w8_a16_moe_block_sigmoid", 8, hidden, router_weight, bias, n_group, topk_group, routed_scaling_factor, top_k,
                     norm_topk_prob, py::none(), gu_w, gu_s, dn_w, dn_s, "auto");
}

Tensor w4_a16_moe_block_sigmoid(const Tensor& hidden, const Tensor& router_weight, const Tensor& bias, int64_t top_k, int64_t n_group,
                                int64_t topk_group, bool norm_topk_prob, double routed_scaling_factor, const Tensor& gu_w,
                                const Tensor& gu_s, const Tensor& dn_w, const Tensor& dn_s, const std::string& path)
{
    TORCH_CHECK(bias.defined(), "w4_a16_moe_block_sigmoid: the correction bias is required");
    return moe_block("w4_a16_moe_block_sigmoid", 4, hidden, router_weight, bias, n_group, topk_group, routed_scaling_factor, top_k,
                     norm_topk_prob, py::none(), gu_w, gu_s, dn_w, dn_s, path);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "EETQ operator module on libeetq_amd.so (MI355X / gfx950)";
    // ---- the reference's six functions (csrc/eetpy.cpp:9-19): names, order, py::arg names and defaults kept ----------
    m.def("w8_a16_gemm", &w8_a16_gemm, "Weight only gemm", py::arg("input"), py::arg("weight"), py::arg("scale"),
          py::arg("path") = "auto", py::arg("bias") = py::none(), py::arg("residual") = py::none(),
          py::arg("norm") = py::none(), py::arg("gated") = false, py::arg("activation") = "");
    m.def("w8_a16_gemm_", &w8_a16_gemm_, "Weight only gemm inplace", py::arg("input"), py::arg("weight"), py::arg("scale"),
          py::arg("output"), py::arg("m"), py::arg("n"), py::arg("k"));
    m.def("preprocess_weights", &preprocess_weights, "transform_int8_weights_for_cutlass", py::arg("origin_weight"),
          py::arg("is_int4") = false, py::arg("layout") = "gfx950");
    m.def("quant_weights", &quant_weights, "quantize weight", py::arg("origin_weight"), py::arg("quant_type"),
          py::arg("return_unprocessed_quantized_tensor") = false, py::arg("layout") = "gfx950");
    m.def("rotary_embedding_neox", &rotary_embedding_neox, "Apply GPT-NeoX style rotary embedding to query and key",
          py::arg("positions"), py::arg("query"), py::arg("key"), py::arg("head_size"), py::arg("cos_sin_cache"));
    m.def("layernorm_forward", &layernorm_forward, "LayerNorm kernel", py::arg("input"), py::arg("gamma"), py::arg("out"),
          py::arg("eps"));
    // ---- extensions of this library ----------------------------------------------------------------------------------
    m.def("w8_a16_gemm_t", &w8_a16_gemm_t, "input gradient of the weight-only gemm: input . dequant(weight)^T",
          py::arg("input"), py::arg("weight"), py::arg("scale"));
    m.def("w4_a16_gemm_t", &w4_a16_gemm_t, "the same from a packed int4 [K, N/2] weight in the gfx950 int4 layout",
          py::arg("input"), py::arg("weight"), py::arg("scale"));
    m.def("w4_a16_gemm_tiled", &w4_a16_gemm_tiled, "W4A16 prompt gemm on the int4 tiles themselves: no expansion, no scratch",
          py::arg("input"), py::arg("weight"), py::arg("scale"), py::arg("bias") = py::none(), py::arg("residual") = py::none(),
          py::arg("tile") = 0);
    m.def("w4_a16_gemm_tiled_supported", &w4_a16_gemm_tiled_supported, "1 where w4_a16_gemm_tiled takes an [M, K] x [K, N] product",
          py::arg("M"), py::arg("N"), py::arg("K"));
    m.def("unprocess_weights", &unprocess_weights, "inverse of preprocess_weights", py::arg("processed_weight"),
          py::arg("layout") = "gfx950", py::arg("is_int4") = false);
    m.def("rotary_embedding_neox_strided", &rotary_embedding_neox_strided, "rotary embedding on strided q/k views",
          py::arg("positions"), py::arg("query"), py::arg("key"), py::arg("head_size"), py::arg("cos_sin_cache"));
    m.def("rotary_embedding_neox_kvcache", &rotary_embedding_neox_kvcache, "decode-step rotary + KV-cache write",
          py::arg("positions"), py::arg("query"), py::arg("key"), py::arg("value"), py::arg("head_size"),
          py::arg("cos_sin_cache"), py::arg("key_cache"), py::arg("value_cache"), py::arg("slots") = py::none(),
          py::arg("ring") = false);
    m.def("rotary_embedding_neox_kvcache_prefill", &rotary_embedding_neox_kvcache_prefill, "prompt rotary + KV-cache write",
          py::arg("positions"), py::arg("query"), py::arg("key"), py::arg("value"), py::arg("head_size"),
          py::arg("cos_sin_cache"), py::arg("key_cache"), py::arg("value_cache"), py::arg("first_row") = 0,
          py::arg("first_row_dev") = py::none(), py::arg("ring") = false);
    m.def("greedy_handover", &greedy_handover, "argmax + token hand-over of a greedy decode step", py::arg("logits"),
          py::arg("out_tokens"), py::arg("column"), py::arg("next_token"), py::arg("position"));
    m.def("sample_handover", &sample_handover, "temperature / top-k / top-p sampling + token hand-over of a decode step",
          py::arg("logits"), py::arg("out_tokens"), py::arg("column"), py::arg("next_token"), py::arg("position"), py::arg("params"),
          py::arg("done") = py::none(), py::arg("uniforms") = py::none());
    m.def("ngram_draft", &ngram_draft, "prompt-lookup draft of a speculative decode step", py::arg("hist"), py::arg("position"),
          py::arg("draft"), py::arg("max_ngram") = 3);
    m.def("spec_accept", &spec_accept, "verify + accept + token hand-over of a speculative decode step", py::arg("logits"),
          py::arg("draft"), py::arg("out_tokens"), py::arg("column"), py::arg("next_token"), py::arg("position"), py::arg("limit"),
          py::arg("hist"), py::arg("stats"));
    m.def("spec_sample_accept", &spec_sample_accept, "verify + accept + token hand-over of a speculative decode step, sampled",
          py::arg("logits"), py::arg("draft"), py::arg("out_tokens"), py::arg("column"), py::arg("next_token"), py::arg("position"),
          py::arg("limit"), py::arg("hist"), py::arg("stats"), py::arg("params"), py::arg("done") = py::none(),
          py::arg("uniforms") = py::none(), py::arg("workspace") = py::none());
    m.def("decode_attention", &decode_attention, "single-query attention over a KV cache", py::arg("query"),
          py::arg("key_cache"), py::arg("value_cache"), py::arg("mask") = py::none(), py::arg("scaling") = py::none(),
          py::arg("splits") = py::none(), py::arg("kv_len") = py::none(), py::arg("kv_len_bias") = 0,
          py::arg("advance") = py::none(), py::arg("kv_start") = py::none(), py::arg("window") = py::none(),
          py::arg("ring") = false);
    m.def("rope_decode_attention", &rope_decode_attention, py::arg("positions"), py::arg("query"), py::arg("key"),
          py::arg("value"), py::arg("cos_sin_cache"), py::arg("key_cache"), py::arg("value_cache"), py::arg("tickets"),
          py::arg("slots") = py::none(), py::arg("mask") = py::none(), py::arg("scaling") = py::none(),
          py::arg("splits") = py::none(), py::arg("kv_len") = py::none(), py::arg("kv_len_bias") = 0,
          py::arg("advance") = py::none(), py::arg("kv_start") = py::none(), py::arg("window") = py::none(),
          py::arg("ring") = false);
    m.def("decode_attention_i8kv", &decode_attention_i8kv, "single-query attention over an int8 KV cache", py::arg("query"),
          py::arg("key_cache"), py::arg("value_cache"), py::arg("scales"), py::arg("mask") = py::none(),
          py::arg("scaling") = py::none(), py::arg("splits") = py::none(), py::arg("kv_len") = py::none(),
          py::arg("kv_len_bias") = 0, py::arg("advance") = py::none());
    m.def("rope_decode_attention_i8kv", &rope_decode_attention_i8kv, py::arg("positions"), py::arg("query"), py::arg("key"),
          py::arg("value"), py::arg("cos_sin_cache"), py::arg("key_cache"), py::arg("value_cache"), py::arg("scales"),
          py::arg("tickets"), py::arg("slots") = py::none(), py::arg("mask") = py::none(), py::arg("scaling") = py::none(),
          py::arg("splits") = py::none(), py::arg("kv_len") = py::none(), py::arg("kv_len_bias") = 0,
          py::arg("advance") = py::none());
    m.def("rotary_embedding_neox_kvcache_prefill_i8", &rotary_embedding_neox_kvcache_prefill_i8,
          "prompt rotary (query and key in place) + quantising int8 KV-cache write", py::arg("positions"), py::arg("query"),
          py::arg("key"), py::arg("value"), py::arg("head_size"), py::arg("cos_sin_cache"), py::arg("key_cache"),
          py::arg("value_cache"), py::arg("scales"), py::arg("first_row") = 0, py::arg("first_row_dev") = py::none());
    m.def("prefill_attention", &prefill_attention, py::arg("query"), py::arg("key"), py::arg("value"), py::arg("keys"),
          py::arg("scaling") = py::none(), py::arg("causal_offset") = py::none(), py::kw_only(), py::arg("kv_len") = py::none(),
          py::arg("kv_len_bias") = 0, py::arg("splits") = py::none(), py::arg("workspace") = py::none(),
          py::arg("kv_start") = py::none(), py::arg("window") = py::none(), py::arg("ring") = false,
          "causal attention of a prompt's query rows [B, T, H, D] over the first `keys` rows of a KV cache [B, Hkv, S, D] (MFMA)");
    m.def("prefill_attention_i8kv", &prefill_attention_i8kv, py::arg("query"), py::arg("key_cache"), py::arg("value_cache"),
          py::arg("scales"), py::arg("max_keys"), py::arg("scaling") = py::none(), py::arg("kv_len") = py::none(),
          py::arg("kv_len_bias") = 0, py::arg("splits") = py::none(), py::arg("workspace") = py::none(),
          py::arg("window") = py::none(), py::arg("ring") = false,
          "prefill_attention behind an int8 KV cache: a prompt's query rows [B, T, H, D] over the dequantised first rows of the cache");
    m.def("decode_attention_rows", &decode_attention_rows, py::arg("query"), py::arg("key"), py::arg("value"), py::arg("keys"),
          py::arg("scaling") = py::none(), py::arg("kv_len") = py::none(), py::arg("kv_len_bias") = 0, py::arg("splits") = py::none(),
          py::arg("workspace") = py::none(), py::arg("ring") = false,
          "1 .. 16 query rows [B, R, H, D], the last rows of the first `keys` rows of a KV cache [B, Hkv, S, D], attending it causally "
          "(split-KV, MFMA)");
    m.def("decode_attention_rows_i8kv", &decode_attention_rows_i8kv, py::arg("query"), py::arg("key_cache"), py::arg("value_cache"),
          py::arg("scales"), py::arg("max_keys"), py::arg("scaling") = py::none(), py::arg("kv_len") = py::none(),
          py::arg("kv_len_bias") = 0, py::arg("splits") = py::none(), py::arg("workspace") = py::none(), py::arg("ring") = false,
          "decode_attention_rows behind an int8 KV cache: 1 .. 16 query rows [B, R, H, D] over the dequantised first rows of the cache");
    m.def("decode_attention_rows_splits", &decode_attention_rows_splits, py::arg("batch"), py::arg("heads"), py::arg("kv_heads"),
          py::arg("rows"), py::arg("max_keys"), "the chunk count decode_attention_rows uses with splits=None");
    m.def("prefill_attention_supported", &prefill_attention_supported, py::arg("head_dim"));
    m.def("prefill_attention_splits", &prefill_attention_splits, py::arg("batch"), py::arg("heads"), py::arg("q_tokens"), py::arg("max_keys"),
          "the split count prefill_attention uses with splits=None (1 = unsplit)");
    m.def("llama_decode_layer", &llama_decode_layer, "one decode step of an accelerated Llama decoder layer (six launches, one call)",
          py::arg("hidden"), py::arg("input_norm"), py::arg("qkv_weight"), py::arg("qkv_scale"), py::arg("qkv_bias"),
          py::arg("positions"), py::arg("cos_sin_cache"), py::arg("key_cache"), py::arg("value_cache"), py::arg("tickets"),
          py::arg("counter"), py::arg("mask"), py::arg("scaling"), py::arg("heads"), py::arg("kv_heads"), py::arg("o_weight"),
          py::arg("o_scale"), py::arg("o_bias"), py::arg("post_norm"), py::arg("gate_up_weight"), py::arg("gate_up_scale"),
          py::arg("gate_up_bias"), py::arg("down_weight"), py::arg("down_scale"), py::arg("down_bias"), py::arg("glu8") = false);
    m.def("silu_mul", &silu_mul, "silu(gate) * up on a fused gate|up block (glu8: columns in groups of 8 gate + 8 up)",
          py::arg("gate_up"), py::arg("glu8") = false);
    m.def("w8_a16_gemv_grouped", &w8_a16_gemv_grouped, "independent single-row W8A16 problems in as few dispatches as possible",
          py::arg("inputs"), py::arg("weights"), py::arg("scales"), py::arg("biases") = py::none(),
          py::arg("residuals") = py::none());
    m.def("w8_a16_moe", &w8_a16_moe, "routed W8A16 mixture-of-experts layer over int8 expert stacks", py::arg("hidden"),
          py::arg("top_k_index"), py::arg("top_k_weights"), py::arg("gate_up_qweight"), py::arg("gate_up_scales"),
          py::arg("down_qweight"), py::arg("down_scales"));
    m.def("w8_a16_moe_train", &w8_a16_moe_train,
          "trainable forward of the routed W8A16 experts layer: (out, routing tables, gate_up, y) for w8_a16_moe_backward",
          py::arg("hidden"), py::arg("top_k_index"), py::arg("top_k_weights"), py::arg("gate_up_qweight"), py::arg("gate_up_scales"),
          py::arg("down_qweight"), py::arg("down_scales"));
    m.def("w8_a16_moe_backward", &w8_a16_moe_backward,
          "input and router-weight gradients of the routed W8A16 experts layer (frozen int8 weights)", py::arg("grad_out"),
          py::arg("top_k_weights"), py::arg("tables"), py::arg("gate_up"), py::arg("y"), py::arg("gate_up_qweight"),
          py::arg("gate_up_scales"), py::arg("down_qweight"), py::arg("down_scales"), py::arg("need_input_grad") = true,
          py::arg("need_weights_grad") = true);
    m.def("w4_a16_moe", &w4_a16_moe,
          "routed W4A16 mixture-of-experts layer over int4 expert stacks (the inference forward); path: 'auto', 'decode', 'expand' or "
          "'direct'",
          py::arg("hidden"), py::arg("top_k_index"), py::arg("top_k_weights"), py::arg("gate_up_qweight"), py::arg("gate_up_scales"),
          py::arg("down_qweight"), py::arg("down_scales"), py::arg("path") = "auto");
    m.def("w4_a16_moe_train", &w4_a16_moe_train,
          "trainable forward of the routed W4A16 experts layer: (out, routing tables, gate_up, y) for w4_a16_moe_backward; path as "
          "w4_a16_moe",
          py::arg("hidden"), py::arg("top_k_index"), py::arg("top_k_weights"), py::arg("gate_up_qweight"), py::arg("gate_up_scales"),
          py::arg("down_qweight"), py::arg("down_scales"), py::arg("path") = "auto");
    m.def("w4_a16_moe_backward", &w4_a16_moe_backward,
          "input and router-weight gradients of the routed W4A16 experts layer (frozen int4 weights, read as int4 tiles)",
          py::arg("grad_out"), py::arg("top_k_weights"), py::arg("tables"), py::arg("gate_up"), py::arg("y"), py::arg("gate_up_qweight"),
          py::arg("gate_up_scales"), py::arg("down_qweight"), py::arg("down_scales"), py::arg("need_input_grad") = true,
          py::arg("need_weights_grad") = true);
    m.def("w4_a16_moe_path", &w4_a16_moe_path,
          "'decode' or 'expand': the grouped kernels w4_a16_moe(path='auto') runs for T tokens, k choices, E experts, H, I",
          py::arg("T"), py::arg("k"), py::arg("E"), py::arg("H"), py::arg("I"));
    m.def("w4_a16_moe_direct_supported", &w4_a16_moe_direct_supported,
          "True where w4_a16_moe(path='direct') takes T tokens, k choices, E experts, H, I (the grouped int4 tiled kernel's limits)",
          py::arg("T"), py::arg("k"), py::arg("E"), py::arg("H"), py::arg("I"));
    const py::object f32 = py::module_::import("torch").attr("float32");
    m.def("moe_router", &moe_router,
          "transformers' TopKRouter forward on the device: (router_logits fp16 [T, E], router_scores [T, k], router_indices int64 [T, k])",
          py::arg("hidden"), py::arg("weight"), py::arg("top_k"), py::arg("norm_topk_prob") = true, py::arg("scores_dtype") = f32);
    m.def("w8_a16_moe_block", &w8_a16_moe_block, "router + routed W8A16 experts: the whole sparse MoE block (four launches at T <= 16)",
          py::arg("hidden"), py::arg("router_weight"), py::arg("top_k"), py::arg("norm_topk_prob"), py::arg("scores_dtype"),
          py::arg("gate_up_qweight"), py::arg("gate_up_scales"), py::arg("down_qweight"), py::arg("down_scales"));
    m.def("w4_a16_moe_block", &w4_a16_moe_block,
          "router + routed W4A16 experts: the whole sparse MoE block (inference only); path: 'auto', 'decode', 'expand' or 'direct'",
          py::arg("hidden"), py::arg("router_weight"), py::arg("top_k"), py::arg("norm_topk_prob"), py::arg("scores_dtype"),
          py::arg("gate_up_qweight"), py::arg("gate_up_scales"), py::arg("down_qweight"), py::arg("down_scales"), py::arg("path") = "auto");
    m.def("moe_router_sigmoid", &moe_router_sigmoid,
          "transformers' DeepseekV3TopkRouter forward on the device: (router_logits fp32 [T, E], top_k_weights fp32 [T, k], top_k_index "
          "int64 [T, k])",
          py::arg("hidden"), py::arg("weight"), py::arg("bias"), py::arg("top_k"), py::arg("n_group"), py::arg("topk_group"),
          py::arg("norm_topk_prob"), py::arg("routed_scaling_factor"));
    m.def("w8_a16_moe_block_sigmoid", &w8_a16_moe_block_sigmoid,
          "sigmoid group-limited router + routed W8A16 experts (four launches at T <= 16; the shared expert is the caller's)",
          py::arg("hidden"), py::arg("router_weight"), py::arg("bias"), py::arg("top_k"), py::arg("n_group"), py::arg("topk_group"),
          py::arg("norm_topk_prob"), py::arg("routed_scaling_factor"), py::arg("gate_up_qweight"), py::arg("gate_up_scales"),
          py::arg("down_qweight"), py::arg("down_scales"));
    m.def("w4_a16_moe_block_sigmoid", &w4_a16_moe_block_sigmoid,
          "sigmoid group-limited router + routed W4A16 experts (inference only; the shared expert is the caller's); path: 'auto', "
          "'decode', 'expand' or 'direct'",
          py::arg("hidden"),
          py::arg("router_weight"), py::arg("bias"), py::arg("top_k"), py::arg("n_group"), py::arg("topk_group"),
          py::arg("norm_topk_prob"), py::arg("routed_scaling_factor"), py::arg("gate_up_qweight"), py::arg("gate_up_scales"),
          py::arg("down_qweight"), py::arg("down_scales"), py::arg("path") = "auto");
    m.attr("__eetq_amd_version__") = eetq_version();
}
