// Descriptor -> log-plan in one call (cost build feeding the OT solve).
//   variant 1: first_layer.py:110-115   (einsum, /sqrt(D), 0.1*, log_optimal_transport)
//   variant 2: second_layer.py:100-105 / third_layer.py:156-158 (log_optimal_transport2)
// The score matrix lives only in the caller's workspace (L2 / Infinity-Cache resident between the
// MFMA kernel and the Sinkhorn kernel on the same stream); nothing is returned to the host side.
#include "launch.hpp"

using namespace pats;


// Measurement hook (bench.py): an event the next cost_ot call of THIS THREAD records between its two launches (cost build |
// Sinkhorn), so that the two kernels of the one C call can be timed inside a step instead of on their own afterwards.
static thread_local hipEvent_t g_mid_event = nullptr;
extern "C" int pats_set_cost_ot_mid_event(void* event) {
    g_mid_event = (hipEvent_t)event;
    return PATS_OK;
}

extern "C" size_t pats_cost_ot_workspace_bytes(int64_t batch, int D, int n, int m, int variant) {
    (void)D;
    if (variant == 2 && n == 65 && m == 65 && (D % 32) == 0 && D <= 512) return 0;
    const size_t scores = align256((size_t)batch * n * m * sizeof(float));
    const int M = variant == 1 ? n + 1 : n, N = variant == 1 ? m + 1 : m;
    return scores + (variant == 1 ? pats_ot_workspace_bytes(batch, M, N) : pats_ot2_workspace_bytes(batch, M, N));
}

// d0 / d1: descriptors of `dtype` elements (pats_map_dtype_t)
static int cost_ot_impl(const void* d0, const void* d1, int dtype, int64_t batch, int D, int n, int m, int variant,
                        const float* scalar, const float* ns, int iters, float bias_k, float* Z, uint8_t* col_nomatch,
                        void* workspace, size_t workspace_bytes, pats_stream_t stream, const int64_t* live = nullptr);

extern "C" int pats_cost_ot_f32(const float* d0, const float* d1, int64_t batch, int D, int n, int m,
                                int variant, const float* scalar, const float* ns, int iters,
                                float bias_k, float* Z, void* workspace, size_t workspace_bytes,
                                pats_stream_t stream) {
    return cost_ot_impl(d0, d1, PATS_MAP_F32, batch, D, n, m, variant, scalar, ns, iters, bias_k, Z, nullptr, workspace,
                        workspace_bytes, stream);
}

// variant 2 only: additionally est_position's if_nomatching2 (second_layer.py:243,248) from the OT epilogue
extern "C" int pats_cost_ot_flags_f32(const float* d0, const float* d1, int64_t batch, int D, int n, int m,
                                      int variant, const float* scalar, const float* ns, int iters,
                                      float bias_k, float* Z, uint8_t* col_nomatch, void* workspace,
                                      size_t workspace_bytes, pats_stream_t stream) {
    PATS_REQUIRE(variant == 2, "cost_ot_flags: column flags come from the log_optimal_transport2 epilogue (variant 2); "
                               "for variant 1 use pats_colmass_flags_f32, which the coarse level needs anyway");
    return cost_ot_impl(d0, d1, PATS_MAP_F32, batch, D, n, m, variant, scalar, ns, iters, bias_k, Z, col_nomatch, workspace,
                        workspace_bytes, stream);
}

// The fine level of a batch whose row count lives on the device (throughput mode: the row table's total, pats_chunk_rows_device):
// launched over the capacity `batch_cap`, the workgroups of problems >= *batch_dev return at once - no cost build, no solve, no
// log-domain redo; their Z / col_nomatch rows are left untouched.
extern "C" int pats_cost_ot_flags_counted_f32(const float* d0, const float* d1, int64_t batch_cap, const int64_t* batch_dev,
                                              int D, int n, int m, int variant, const float* scalar, const float* ns, int iters,
                                              float bias_k, float* Z, uint8_t* col_nomatch, void* workspace,
                                              size_t workspace_bytes, pats_stream_t stream) {
    PATS_REQUIRE(variant == 2 && n == 145 && m == 145, "cost_ot_flags_counted: the fine level only (variant 2, 145 x 145)");
    PATS_REQUIRE(batch_dev, "cost_ot_flags_counted: null count");
    return cost_ot_impl(d0, d1, PATS_MAP_F32, batch_cap, D, n, m, variant, scalar, ns, iters, bias_k, Z, col_nomatch, workspace,
                        workspace_bytes, stream, batch_dev);
}

// The three entries above in one, on descriptors of any pats_map_dtype_t (widened to fp32 at the cost build's loads: same
// bits as on .float() copies).  col_nomatch (nullable): the variant-2 column flags; batch_dev (nullable): the fine level's
// device-side row count.  Half descriptors at the fine level take the two-kernel path whatever pats_set_fine_fused says.
extern "C" int pats_cost_ot_typed(const void* d0, const void* d1, pats_map_dtype_t dtype, int64_t batch_cap,
                                  const int64_t* batch_dev, int D, int n, int m, int variant, const float* scalar,
                                  const float* ns, int iters, float bias_k, float* Z, uint8_t* col_nomatch, void* workspace,
                                  size_t workspace_bytes, pats_stream_t stream) {
    PATS_REQUIRE(known_elem_type((int)dtype), "cost_ot_typed: unknown descriptor dtype %d", (int)dtype);
    PATS_REQUIRE(!col_nomatch || variant == 2, "cost_ot_typed: column flags come from the log_optimal_transport2 epilogue (variant 2)");
    PATS_REQUIRE(!batch_dev || (variant == 2 && n == 145 && m == 145 && col_nomatch),
                 "cost_ot_typed: a device-side count is taken at the fine level only (variant 2, 145 x 145, with column flags)");
    if (batch_cap > 0) {
        PATS_REQUIRE(d0 && d1 && ns && Z, "cost_ot_typed: null pointer");
        PATS_REQUIRE((uintptr_t)d0 % desc_elem_bytes((int)dtype) == 0 && (uintptr_t)d1 % desc_elem_bytes((int)dtype) == 0,
                     "cost_ot_typed: descriptors must be aligned to their element size (%d bytes)", (int)desc_elem_bytes((int)dtype));
    }
    return cost_ot_impl(d0, d1, (int)dtype, batch_cap, D, n, m, variant, scalar, ns, iters, bias_k, Z, col_nomatch, workspace,
                        workspace_bytes, stream, batch_dev);
}

static int cost_ot_impl(const void* d0, const void* d1, int dtype, int64_t batch, int D, int n, int m, int variant,
                        const float* scalar, const float* ns, int iters, float bias_k, float* Z, uint8_t* col_nomatch,
                        void* workspace, size_t workspace_bytes, pats_stream_t stream, const int64_t* live) {
    // the handle is consumed by THIS call whatever path it takes (fused kernel, 65-wide kernel, an error): left armed it would be
    // recorded by a later, unrelated call - by then possibly destroyed (round-4 advice)
    const hipEvent_t mid_event = g_mid_event;
    g_mid_event = nullptr;
    PATS_REQUIRE(variant == 1 || variant == 2, "cost_ot: variant must be 1 or 2");
    PATS_REQUIRE(batch >= 0 && D > 0 && n > 0 && m > 0, "cost_ot: bad shape");
    if (batch == 0) return PATS_OK;
    if (variant == 2 && n == 65 && m == 65 && (D % 32) == 0 && D <= 512) {
        PATS_REQUIRE(d0 && d1 && ns && Z, "cost_ot: null pointer");
        int rc = launch_cost_ot65(d0, d1, dtype, batch, D, scalar, ns, iters, bias_k, Z, stream);
        if (!rc && col_nomatch) rc = launch_col_flags(Z, batch, n, m, col_nomatch, nullptr, (hipStream_t)stream);
        return rc;
    }
    PATS_REQUIRE(workspace && workspace_bytes >= pats_cost_ot_workspace_bytes(batch, D, n, m, variant),
                 "cost_ot: workspace too small");
    float* scores = (float*)workspace;
    const size_t off = align256((size_t)batch * n * m * sizeof(float));
    void* ws2 = (char*)workspace + off;
    if (variant == 2 && n == 145 && m == 145 && dtype == PATS_MAP_F32) {
        // the fine level: cost build and OT in ONE kernel, the score matrix never reaches HBM (sinkhorn_blk.hip, FUSED);
        // the guard flags sit where the unfused path keeps them.  (float32 descriptors only: half ones take the two kernels
        // below, which the fused kernel is held to bit for bit.)
        PATS_REQUIRE(d0 && d1 && ns && Z, "cost_ot: null pointer");
        bool applied = false;
        int rc = launch_fine145_fused((const float*)d0, (const float*)d1, D, batch, ns, scalar, iters, bias_k, Z, (int*)ws2, col_nomatch, (hipStream_t)stream,
                                      &applied, live);
        if (rc || applied) return rc;
    }
    // float32: the call the _f32 entries always made; half types: validated by pats_cost_ot_typed
    int rc = dtype == PATS_MAP_F32 ? launch_cost((const float*)d0, (const float*)d1, batch, D, n, m, scores, stream, live)
                                   : launch_cost_typed(d0, d1, dtype, batch, D, n, m, scores, stream, live);
    if (rc) return rc;
    if (mid_event && hipEventRecord(mid_event, (hipStream_t)stream) != hipSuccess) return check_launch("cost_ot mid event");
    if (variant == 1) {
        PATS_REQUIRE(scalar, "cost_ot: alpha pointer required for variant 1");
        PATS_REQUIRE(bias_k == 0.f, "cost_ot: bias only applies to variant 2");
        return pats_log_optimal_transport_f32(scores, batch, n, m, scalar, ns, iters, Z, ws2,
                                              workspace_bytes - off, stream);
    }
    return ot2_flags_live(scores, batch, n, m, scalar, ns, iters, bias_k, Z, col_nomatch, ws2, workspace_bytes - off, stream, live);
}
