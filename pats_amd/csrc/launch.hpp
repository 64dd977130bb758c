// The internal interface of the front end (Sinkhorn solvers, cost builds, GNN layers): every function that one translation unit
// defines and another calls is declared HERE, once, grouped by the file that defines it.  The defining file includes this header
// too, so the compiler holds each definition to the declaration its callers use; default arguments exist only here.  (The
// third-level launchers take Fused65Args and are declared beside it in third_device.hpp; what host.cpp offers every file -
// set_error, check_launch, sinkhorn_mode, ... - is in common.hpp.)  Declarations only: nothing is wrapped.
#pragma once
#include "common.hpp"

namespace pats {

// host.cpp
bool fine_fused();       // pats_set_fine_fused / PATS_FINE_FUSED

// post.hip
int launch_col_flags(const float* Z, int64_t batch, int M, int N, uint8_t* col_nomatch, const int* only_if, hipStream_t st);

// cost.hip (live: optional device-side problem count)
int launch_cost(const float* d0, const float* d1, int64_t batch, int D, int n, int m, float* out, pats_stream_t stream,
                const int64_t* live);
int launch_cost_typed(const void* d0, const void* d1, int dtype, int64_t batch, int D, int n, int m, float* out,
                      pats_stream_t stream, const int64_t* live);

// sinkhorn.hip (launch_cost65: instantiated there for float, _Float16 and bf16_t)
template <typename T> int launch_cost65(const T* d0, const T* d1, int D, int64_t P, float* out, hipStream_t st);
int launch_cost_ot65(const void* d0, const void* d1, int dtype, int64_t batch, int D, const float* one, const float* ns, int iters,
                     float bias_k, float* Z, pats_stream_t stream);
int launch_fine145_fused(const float* d0, const float* d1, int D, int64_t batch, const float* ns, const float* one, int iters,
                         float bias_k, float* out, int* fail, uint8_t* col_nomatch, hipStream_t st, bool* applied,
                         const int64_t* live);
int ot2_flags_live(const float* scores, int64_t batch, int m, int n, const float* one, const float* ns, int iters, float bias_k,
                   float* Z, uint8_t* col_nomatch, void* workspace, size_t workspace_bytes, pats_stream_t stream,
                   const int64_t* live);

// sinkhorn_stream.hip
size_t stream_workspace_bytes(int64_t batch, int M, int N);
int launch_stream(const float* base, int64_t stride, int ld, int rows, int cols, const float* alpha, int64_t batch, int M, int N,
                  const float* log_mu, const float* log_nu, const float* norm, int iters, float* out, void* ws, int* fail,
                  hipStream_t st);

// sinkhorn_blk.hip
int launch_blk145(int mode, const float* Z, int64_t batch, const float* log_mu, const float* log_nu, const float* ns,
                  const float* one, int iters, float bias_k, float* out, int* fail, uint8_t* col_nomatch, hipStream_t st,
                  const int64_t* live = nullptr);
int launch_blk145_fused(const float* d0, const float* d1, int D, int64_t batch, const float* ns, const float* one, int iters,
                        float bias_k, float* out, int* fail, uint8_t* col_nomatch, hipStream_t st, const int64_t* live);

// sinkhorn_blk2w.hip: the two-wave form of the same kernel
bool fine_w2_enabled();
int launch_blk145_w2(int mode, const float* Z, int64_t batch, const float* log_mu, const float* log_nu, const float* ns,
                     const float* one, int iters, float bias_k, float* out, int* fail, uint8_t* col_nomatch, hipStream_t st,
                     const int64_t* live);

// attention.hip
int launch_attention(const float* query, const float* key, const float* value, int64_t batch, int dim, int heads, int n, int m,
                     float* out, float* prob, pats_stream_t stream, const int* gate);

// attention145.hip
int launch_attention145(const float* query, const float* key, const float* value, int64_t batch, int dim, int heads, int n, int m,
                        float* out, int* flag, const int* gate, hipStream_t st);

// conv_pk.hip (`redo`: one int of workspace, zero on entry - conv_lean_kernel of gnn.hip raises it; null -> conv1x1_kernel only)
size_t conv_packed_bytes(int K, int M);
int launch_conv_pack(const float* wt, int K, int M, void* packed, hipStream_t st);
bool conv_pk_ready();
int launch_conv_pk(const void* packed, const float* x0, const float* x1, int K0, int K1, int M, int n, int64_t cols,
                   const float* in_scale, const float* in_shift, const float* bias, const float* residual, float* y, int* redo,
                   const int* gate, hipStream_t st, int layout);

// gnn_fused.hip
int fused_layer_supported(int C, int heads, int n, int m);
size_t packed_fused_bytes(int C, int heads);
bool gnn_fold_enabled();                                                     // (merge folded into mlp[0])
const float* packed_folded_bias(const void* packed, int C, int heads);
const void* packed_fine_section(const void* packed, int C, int heads);
int launch_fused_layer(const float* x, const float* source, int64_t batch, const void* packed, const float* bn_a, const float* bn_b,
                       int bn_train, const float* residual, float* out, float* hid, int* flag, double* bn_part, int* splits_out,
                       hipStream_t st, const int64_t* live = nullptr, int64_t live_off = 0);
int launch_gnn_tail(const float* hid, int64_t batch, const void* packed, const float* scale, const float* shift, const float* residual,
                    float* out, int* flag, hipStream_t st);

// gnn_fine.hip: the fine level's one-kernel layer
int fine_layer_supported(int C, int heads, int n, int m);
size_t packed_fine_bytes(int C, int heads);
int launch_fine_pack(const pats_propagation_weights& w, void* section, hipStream_t st);
size_t fine_scratch_bytes(int64_t P);
size_t fine_image_bytes(int64_t P);
int launch_fine_in(const float* x, int64_t P, char* tf, hipStream_t st);
int launch_fine_out(const char* tf, int64_t P, float* y, hipStream_t st, const int64_t* live = nullptr, int64_t live_off = 0,
                    const float* add = nullptr);
int launch_fine_layer(const char* tf_x, const char* tf_s, int64_t shift, int residual, int64_t P, const void* section,
                      char* tf_out, char* tf_att, char* qkv, int* flag, const int* gate, hipStream_t st, int sets,
                      const int64_t* live, int64_t live_off);
int launch_fine_qkv(const char* tf, int64_t P, const void* section, char* qkv, int want_q, int want_kv, const int* gate, hipStream_t st,
                    int sets, const int64_t* live, int64_t live_off);
int launch_fine_attn(const char* qkv, int64_t shift, char* tf_att, int64_t P, const int* gate, hipStream_t st, int sets,
                     const int64_t* live, int64_t live_off);
int launch_fine_mlp(const char* tf_x, const char* tf_att, int residual, const void* section, char* tf_out, const void* next_section,
                    char* qkv, int64_t P, int* flag, const int* gate, hipStream_t st, int sets, const int64_t* live, int64_t live_off);

}  // namespace pats
