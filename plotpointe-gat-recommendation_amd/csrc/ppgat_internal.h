// Internal declarations shared by the kernel, graph and ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/ppgat.h"

namespace ppgat {

constexpr int kModePyg = 0;
constexpr int kModeCustom = 1;
constexpr int kMaxHeads = 8;
#ifndef PPGAT_EPI_BLOCKS
#define PPGAT_EPI_BLOCKS 1024
#endif
constexpr int64_t kEpiMaxBlocks = PPGAT_EPI_BLOCKS;
constexpr int kShortItemEdges = 16;  // include/ppgat.h PPGAT_SHORT_ITEM_EDGES

hipError_t launch_stream_copy(const void* src, void* dst, int64_t n_bytes, hipStream_t st);
hipError_t launch_scores(const float* h, const float* as, const float* ad, int64_t n, int heads, int C, float* ss,
                         float* sd, hipStream_t st);
hipError_t launch_fwd(const ppgat_schedule& sch, const int32_t* col, const int32_t* eid, int heads, int C,
                      const float* h, const float* ss, const float* sd, const float* bias, int mode, float slope,
                      float eps, float p, uint64_t seed, uint64_t* seed_out, float* out, float* m, float* invl,
                      float* agg, float* partial, hipStream_t st, const float* et = nullptr);
hipError_t launch_bwd_pro(const float* go, const float* out, const float* agg, const float* bias, const float* sd,
                          const float* m, const float* invl, int64_t n, int heads, int C, float gscale,
                          float* nstate, float* bias_part, int64_t blocks, hipStream_t st);
hipError_t launch_bwd_src(const ppgat_schedule& sch, const int32_t* row, const int32_t* csc_eid, const int32_t* csc2csr,
                          int heads, int C, const float* h, const float* ss, const float* nstate, const float* go,
                          int mode, float slope, float gscale, float p, uint64_t seed, const uint64_t* seed_in,
                          float* dh, int64_t ld_dh, float* ds_src, int64_t ld_ds, float* dz, float* partial,
                          hipStream_t st, const float* et = nullptr);
// gather skipping in launch_fwd / launch_bwd_src (ppgat_set_gather_skip): the current value, and
// set-and-return-previous
int gather_skip();
int set_gather_skip(int on);
// edge features (ppgat_egat.hip): attribute staging, per-step logit terms, the dv reduction
hipError_t edge_attr_permute(const float* attr, const int32_t* eid, int64_t E, int D, float* out, hipStream_t st);
hipError_t edge_terms(const float* attr_csr, const float* attr_csc, const float* v, int64_t E, int D, int H,
                      float* t_csr, float* t_csc, hipStream_t st);
int64_t edge_dv_blocks(int64_t E);
hipError_t edge_dv(const float* dz, const float* attr, int64_t E, int H, int D, float* dv, float* part,
                   hipStream_t st);
hipError_t launch_dst_sum(const ppgat_schedule& sch, int heads, const float* dz, const int32_t* csr2csc, float* ds_dst,
                          int64_t ld, float* partial, hipStream_t st);
hipError_t launch_invert_index(const int32_t* p, int64_t n, int32_t* inv, hipStream_t st);
int64_t epi_blocks(int64_t n);
hipError_t launch_bwd_epi(const int32_t* rowptr, int64_t n, int heads, int C, const float* h, const float* as,
                          const float* ad, const float* ds_src, const float* dz, float* dh, float* partial,
                          int64_t blocks, hipStream_t st);
hipError_t launch_col_reduce(const float* partial, int64_t rows, int cols, int split, float* out_a, float* out_b,
                             hipStream_t st);

// graph preprocessing (ppgat_graph.hip)
size_t csr_workspace_bytes(int64_t n_nodes, int64_t n_edges);
hipError_t csr_build(const int64_t* edge_index, int64_t E, int64_t N, int32_t* rowptr, int32_t* col, int32_t* csr_eid,
                     int32_t* colptr, int32_t* row, int32_t* csc_eid, int32_t* csc2csr, int32_t* bad,
                     void* ws, size_t ws_bytes, hipStream_t st);
int64_t schedule_capacity(int64_t n_nodes, int64_t n_edges, int32_t max_edges);
size_t schedule_workspace_bytes(int64_t n_nodes);
hipError_t schedule_build(const int32_t* ptr, int64_t N, int32_t T, int32_t* item_row, int32_t* item_beg,
                          int32_t* item_end, int32_t* hub_row, int32_t* hub_ptr, int32_t* counts, void* ws,
                          size_t ws_bytes, hipStream_t st);

// training-step kernels (ppgat_train.hip)
bool bpr_channels_ok(int C);
// the backward prologue of the layer that produced Z (heads = 1), fused into the loss backward
struct BprProducer {
  const float* bias;  // nullable
  const float* s_dst;
  const float* m;
  const float* inv_l;
  float gscale;
  float* nstate;      // [n_rows, 4]
  float* grad_bias;   // nullable: [C]
};
size_t bpr_workspace_bytes(int64_t N, int64_t S, int C);
hipError_t bpr_fwd(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, const int32_t* row_map, int C,
                   const int64_t* u, const int64_t* i, const int64_t* j, int64_t S, int kind, float* loss,
                   float* coef, int32_t* bad, void* ws, hipStream_t st);
hipError_t bpr_bwd(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, const int32_t* row_map, int C,
                   const int64_t* u, const int64_t* i, const int64_t* j, int64_t S, const float* coef,
                   const float* grad_loss, float* dZ, void* ws, size_t ws_bytes, hipStream_t st,
                   const BprProducer* prod = nullptr);
hipError_t bpr_bwd_prepare(int64_t n_rows, int64_t n_users, int64_t n_items, const int32_t* row_map, int C,
                           const int64_t* u, const int64_t* i, const int64_t* j, int64_t S, void* ws,
                           size_t ws_bytes, hipStream_t st);
hipError_t bpr_bwd_finish(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, const int32_t* row_map,
                          int C, const int64_t* u, const int64_t* i, const int64_t* j, int64_t S, const float* coef,
                          const float* grad_loss, float* dZ, void* ws, size_t ws_bytes, hipStream_t st,
                          const BprProducer* prod = nullptr);
// the stable LSD radix sort of (key, value) int32 pairs of the loss backwards (keys < 2^bits):
// sorts (k0, v0) with (k1, v1) as the ping-pong pair, *result_in_1 says where the result ended
// (after an odd number of passes: ceil(bits / 10)); mark != NULL: the last pass also sets
// mark[k] = 1 for every key k < mark_n.  ws: rs_workspace_bytes(n, bits).
size_t rs_workspace_bytes(int64_t n, unsigned bits);
hipError_t rs_sort(int32_t* k0, int32_t* v0, int32_t* k1, int32_t* v1, int64_t n, unsigned bits, void* ws,
                   bool* result_in_1, hipStream_t st, uint8_t* mark = nullptr, int64_t mark_n = 0);

// sampled-softmax loss (ppgat_ssm.hip): cand [S, K1], column 0 the positive; n_rows = n_users + n_items;
// corr [n_items] nullable: subtracted from the logits of columns >= 1
size_t ssm_workspace_bytes(int64_t N, int64_t S, int K1, int C);
hipError_t ssm_fwd(const float* Z, int64_t n_users, int64_t n_items, int C, const int64_t* u, const int64_t* cand,
                   const float* corr, int64_t S, int K1, float tau, float* loss, float* coef, int32_t* bad, void* ws,
                   hipStream_t st);
hipError_t ssm_bwd(const float* Z, int64_t n_users, int64_t n_items, int C, const int64_t* u, const int64_t* cand,
                   int64_t S, int K1, const float* coef, const float* grad_loss, float* dZ, void* ws,
                   hipStream_t st);

size_t gemm_tn_workspace_bytes(int64_t N, int M, int K, int nv);
hipError_t gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t N, int M, int K, float* out,
                   float* colsum, const float* V, int64_t ldv, int nv, float* vout, void* ws, hipStream_t st);

// projection GEMMs, weight gradients, optimizer (ppgat_gemm.hip)
bool proj_shape_ok(int K, int ncols);
hipError_t proj_fwd(const float* x0, int64_t ldx0, const float* x1, int64_t ldx1, int64_t split, int64_t n, int K,
                    const float* W, int64_t ldw, const float* bias, const float* att_src, const float* att_dst,
                    float* y, int64_t ldy, float* s_src, float* s_dst, hipStream_t st);
hipError_t proj_dx(const float* D, int64_t ldd, int64_t n, int K, const float* W, int64_t ldw, const float* att_src,
                   const float* att_dst, const float* S, int64_t lds, float* y, int64_t ldy, hipStream_t st);
bool tn128_shape_ok(int M, int K, int nv, const float* V, int64_t ldv);
size_t tn128_workspace_bytes(int64_t N);
hipError_t tn128(const float* A, int64_t lda, const float* B, int64_t ldb, const float* B1, int64_t ldb1, int64_t split,
                 int64_t N, int M, int K, float* out, float* colsum, const float* V, int64_t ldv, int nv, float* vout,
                 void* ws, hipStream_t st);
hipError_t wgrad_assemble(const float* G, const float* GV, const float* W, const float* att_src, const float* att_dst,
                          int heads, int C, int K, float* dW, float* datt_src, float* datt_dst, hipStream_t st);
bool dxw_ok(int hc, int k);
size_t dxw_workspace_bytes(int64_t n);
// the backward prologue of the layer that produced x (heads = 1), fused into k_dxw's epilogue
struct DxwProducer {
  const float* bias;  // nullable
  const float* s_dst;
  const float* m;
  const float* inv_l;
  float gscale;
  float* nstate;      // [n, 4]
  float* grad_bias;   // nullable: [128]
};
hipError_t dxw(const float* D, int64_t ldd, const float* S, int64_t lds, const float* x0, int64_t ldx0, const float* x1,
               int64_t ldx1, int64_t split, int64_t n, const float* W, int64_t ldw, const float* att_src,
               const float* att_dst, float* dx, int64_t lddx, float* G, float* GV, void* ws, hipStream_t st,
               const DxwProducer* prod = nullptr);
int adam_max_tensors();
hipError_t dropout_epoch(int set, uint64_t value, hipStream_t st);
// replicated-item merge (ppgat_dist.hip): phase 0 max, 1 pack, 2 finish
hipError_t rep_merge(int phase, const int32_t* rowptr, int64_t n, int heads, int C, float eps, float* out, float* agg,
                     const float* bias, float* m, float* invl, float* mx, float* pack_a, float* pack_c,
                     hipStream_t st);
// halo exchange rows (ppgat_dist.hip)
hipError_t rows_gather(const float* src, int64_t lds, const int64_t* idx, int64_t n, int cols, float* dst,
                       int64_t ldd, hipStream_t st);
hipError_t rows_return_add(float* dst, int64_t ldd, const float* ret, int64_t ldr, const int32_t* ptr,
                           const int32_t* pos, int64_t n, int cols, hipStream_t st);
hipError_t adam_step(int count, float* const* p, const float* const* g, float* const* m, float* const* v,
                     const int64_t* n, const float* step_size, const float* bc2_sqrt, double beta1, double beta2,
                     float eps, float wd, const float* const* tstep, double lr, hipStream_t st);
// row-sparse Adam: adam_step's element rule on rows[0 .. n_rows) of a [n_table, dim] table (ppgat_gemm.hip)
hipError_t adam_rows(float* p, float* m, float* v, const float* g, const int64_t* rows, int64_t n_rows,
                     int64_t n_table, int dim, float step_size, float bc2_sqrt, double beta1, double beta2, float eps,
                     float wd, int* flag, hipStream_t st);

// I-I kNN neighbour selection (ppgat_knn.hip)
int knn_max_k();
hipError_t knn_topk(const float* S, int64_t ld, int64_t rows, int64_t n_cols, int64_t q0, int k, float min_sim,
                    int32_t* out_idx, float* out_sim, int32_t* out_cnt, hipStream_t st);

// BPR triple sampler (ppgat_sample.hip)
size_t bpr_sampler_workspace_bytes(int64_t n_users, int64_t nnz);
hipError_t bpr_sampler_prepare(const int64_t* ptr, const int32_t* items, int64_t n_users, int64_t nnz,
                               int32_t* items_sorted, int32_t* eligible, int64_t* n_eligible, void* ws,
                               size_t ws_bytes, hipStream_t st);
hipError_t bpr_sample(const int64_t* ptr, const int32_t* items_sorted, const int32_t* eligible,
                      const int64_t* n_eligible, int64_t n_items, int64_t S, uint64_t seed, int64_t t0, int64_t* u,
                      int64_t* i, int64_t* j, int32_t* bad, hipStream_t st);

hipError_t bpr_sample_positives(const int64_t* ptr, const int32_t* items_orig, const int32_t* items_sorted,
                                int64_t n_users, int64_t n_items, int64_t neg_per_pos, int64_t S, uint64_t seed,
                                int64_t t0, int64_t* u, int64_t* i, int64_t* j, int32_t* bad, hipStream_t st);

// LightGCN propagation hop (ppgat_lgcn.hip); src1 / acc1 == NULL: one segment
bool lgcn_channels_ok(int C);
size_t lgcn_workspace_bytes(int64_t n_hub_items, int C);
hipError_t lgcn_hop(const ppgat_schedule& sch, const int32_t* col, const float* val, int C, const float* src0,
                    const float* src1, int64_t src_split, const float* acc0, const float* acc1, int64_t acc_split,
                    float div, float* out, float* accw, float* partial, hipStream_t st);

// GATv2 dynamic-attention layer (ppgat_gatv2.hip); seed: the device slot holding the effective
// mask seed (read when p > 0)
bool gatv2_shape_ok(int H, int C);
size_t gatv2_fwd_workspace_bytes(int64_t n_hub_items, int H, int C);
size_t gatv2_bwd_workspace_bytes(int64_t n, int64_t src_hub_items, int64_t dst_hub_items, int H, int C);
hipError_t gatv2_fwd(const ppgat_schedule& sch, const int32_t* col, const int32_t* eid, int H, int C,
                     const float* xl, const float* xr, const float* att, const float* bias, float slope, float p,
                     const uint64_t* seed, float* out, float* m, float* invl, float* partial, hipStream_t st);
hipError_t gatv2_bwd(const ppgat_schedule& src, const ppgat_schedule& dst, const int32_t* row, const int32_t* csc_eid,
                     const int32_t* col, const int32_t* csr_eid,
                     int64_t n, int H, int C, const float* xl, const float* xr, const float* att, const float* m,
                     const float* invl, const float* g, float slope, float p, const uint64_t* seed, float* dxl,
                     float* dxr, float* datt, float* dbias, void* ws, hipStream_t st);

// attention weights [E, H] from a forward's final state (ppgat_kernels.hip, ppgat_gatv2.hip;
// scatter: at eid[slot] instead of at the slot) and the per-destination selection (ppgat_knn.hip)
hipError_t launch_attention(const ppgat_schedule& sch, const int32_t* col, const int32_t* eid, int heads,
                            const float* ss, const float* sd, const float* m, const float* invl, int mode,
                            float slope, bool scatter, float* alpha, const float* et, hipStream_t st);
hipError_t gatv2_attention(const ppgat_schedule& sch, const int32_t* col, const int32_t* eid, int H, int C,
                           const float* xl, const float* xr, const float* att, const float* m, const float* invl,
                           float slope, bool scatter, float* alpha, hipStream_t st);
hipError_t attention_topk(const int32_t* rowptr, const int32_t* eid, const float* val, int64_t rows, int heads,
                          int k, int32_t* out_eid, float* out_val, int32_t* out_cnt, hipStream_t st);

hipError_t eval_sample(const int64_t* ptr, const int32_t* items_sorted, const int64_t* users, const int64_t* pos,
                       int64_t n_eval, int64_t n_neg, int64_t n_items, uint64_t seed, int64_t* cands, int32_t* bad,
                       hipStream_t st);

// weighted draws (ppgat_sample.hip): cdf [n_items] = inclusive uint64 prefix sum of the quantised
// item weights, cdf[n_items - 1] > 0; the three keep the contracts of their uniform neighbours
hipError_t weighted_draws(const uint64_t* cdf, int64_t n_items, int64_t n, uint64_t seed, int64_t t0, int64_t* out,
                          hipStream_t st);
hipError_t weighted_bpr_sample(const int64_t* ptr, const int32_t* items_sorted, const int32_t* eligible,
                               const int64_t* n_eligible, int64_t n_items, const uint64_t* cdf, int64_t S,
                               uint64_t seed, int64_t t0, int64_t* u, int64_t* i, int64_t* j, int32_t* bad,
                               hipStream_t st);
hipError_t weighted_eval_sample(const int64_t* ptr, const int32_t* items_sorted, const int64_t* users,
                                const int64_t* pos, int64_t n_eval, int64_t n_neg, int64_t n_items,
                                const uint64_t* cdf, uint64_t seed, int64_t* cands, int32_t* bad, hipStream_t st);

// fan-out neighbour sampling (ppgat_nsample.hip): a sampled graph's views compacted out of its
// parent's, no sort.  count -> (host reads info[0] = E') -> sample -> derive, one workspace
// (neighbor_workspace_bytes) carried through the three untouched in between.
constexpr int kMaxFanout = 64;
size_t neighbor_workspace_bytes(int64_t N, int64_t E);
hipError_t neighbor_count(const int32_t* rowptr, int64_t N, int fanout, const int32_t* fanout_of, int32_t* rowptr_s,
                          int32_t* info, void* ws, size_t ws_bytes, hipStream_t st);
hipError_t neighbor_sample(const int32_t* rowptr, const int32_t* col, const int32_t* csr_eid,
                           const int32_t* csr2csc, const int64_t* ei, int64_t N, int64_t E, uint64_t seed,
                           const int32_t* rowptr_s, int64_t Es, int32_t* col_s, int32_t* csr_eid_s, int64_t* ei_s,
                           int64_t* eid, void* ws, size_t ws_bytes, hipStream_t st);
hipError_t neighbor_derive(const int32_t* colptr, const int32_t* row, const int32_t* csc_eid, const int32_t* csc2csr,
                           int64_t N, int64_t E, int64_t Es, int32_t* colptr_s, int32_t* row_s, int32_t* csc_eid_s,
                           int32_t* csc2csr_s, int32_t* csr2csc_s, void* ws, size_t ws_bytes, hipStream_t st);

// seed-subgraph sampling (ppgat_subgraph.hip): the L-hop sampled in-neighbourhood of a seed set.
// seed -> expand (hop 0 .. L - 1) -> plan -> neighbor_count with the plan's cap table -> (host reads
// the two info arrays) -> neighbor_sample -> neighbor_derive -> relabel; one workspace
// (subgraph_workspace_bytes) carried through its own four, untouched in between.
// info [4] = (N_s, n_users_s, bad seed, bad fanout_of entry)
constexpr int kMaxHops = 8;
size_t subgraph_workspace_bytes(int64_t N);
hipError_t subgraph_seed(const int64_t* seeds, int64_t T, int64_t N, int32_t* info, void* ws, size_t ws_bytes,
                         hipStream_t st);
hipError_t subgraph_expand(const int32_t* rowptr, const int32_t* col, int64_t N, int hop, int fanout,
                           const int32_t* fanout_of, uint64_t seed, void* ws, size_t ws_bytes, hipStream_t st);
hipError_t subgraph_plan(int64_t N, int64_t n_users, int hops, int fanout, const int32_t* fanout_of, int32_t* cap,
                         int32_t* info, void* ws, size_t ws_bytes, hipStream_t st);
hipError_t subgraph_relabel(int64_t N, int64_t Ns, int64_t Es, const int64_t* seeds, int64_t T,
                            const int32_t* rowptr_p, const int32_t* colptr_p, int64_t* n_id, int32_t* depth_s,
                            int32_t* rowptr_s, int32_t* colptr_s, int32_t* col_s, int32_t* row_s, int64_t* ei_s,
                            int64_t* seed_local, void* ws, size_t ws_bytes, hipStream_t st);

// evaluation (ppgat_eval.hip)
hipError_t serve_topk(const float* iv, int64_t n_items, int C, const int64_t* hptr, const int64_t* hist,
                      int64_t max_hist, int B, int k, float* U, float* scores, int32_t* out_idx, float* out_score,
                      hipStream_t st);
hipError_t sampled_rank(const float* Z, int64_t n_users, int64_t n_items, const int32_t* row_map, int C,
                        const int64_t* users, const int64_t* cands, int64_t B, int64_t K1, int32_t* rank,
                        hipStream_t st);

// shared-negatives softmax loss (ppgat_shs.hip): one ascending pool [P] scored against every
// sample; uptr / hist nullable together; bad [2] = (out-of-range indices, pool entries out of
// order); the backward takes the workspace the forward left (its mask words)
bool shs_channels_ok(int C);
// corr [n_items] nullable: subtracted from every pool logit; a corrected forward needs the
// shs_corr_workspace_bytes workspace (it keeps corr[pool] behind the uncorrected layout) and its
// backward is called with corrected = true
size_t shs_workspace_bytes(int64_t N, int64_t S, int64_t P, int C);
size_t shs_corr_workspace_bytes(int64_t N, int64_t S, int64_t P, int C);
hipError_t shs_fwd(const float* Z, int64_t n_users, int64_t n_items, int C, const int64_t* u, const int64_t* pos,
                   int64_t S, const int64_t* pool, int64_t P, const int64_t* uptr, const int32_t* hist,
                   const float* corr, float tau, float* loss, float* lse, float* c0, int32_t* bad, void* ws,
                   hipStream_t st);
hipError_t shs_bwd(const float* Z, int64_t n_users, int64_t n_items, int C, const int64_t* u, const int64_t* pos,
                   int64_t S, const int64_t* pool, int64_t P, bool corrected, float tau, const float* lse,
                   const float* c0, const float* grad_loss, float* dZ, void* ws, hipStream_t st);

// full-catalogue ranking (ppgat_fullrank.hip): rank / ties of pos[b] among every item outside
// history(users[b]) + {pos[b]}; uptr / hist nullable together; ties nullable
bool full_rank_channels_ok(int C);
hipError_t full_rank(const float* U, int64_t ldu, int64_t n_users, const float* I, int64_t ldi, int64_t n_items, int C,
                     const int64_t* users, const int64_t* pos, int64_t n_eval, const int64_t* uptr,
                     const int32_t* hist, int32_t* rank, int32_t* ties, hipStream_t st);

// full-catalogue top-K (ppgat_fulltopk.hip): the k best items outside history(users[b]) under
// (score descending, item ascending); users nullable (query b = user b), uptr / hist nullable
// together, out_score nullable.  The workspace depends on the device's CU count (the item range is
// split to fill the chip); _floor is its device-independent lower bound (no split).
bool full_topk_channels_ok(int C);
int full_topk_max_k();
size_t full_topk_workspace_floor(int64_t n_query, int64_t n_items, int C, int k);
hipError_t full_topk_workspace(int64_t n_query, int64_t n_items, int C, int k, size_t* bytes);
hipError_t full_topk(const float* U, int64_t ldu, int64_t n_users, const float* I, int64_t ldi, int64_t n_items, int C,
                     const int64_t* users, int64_t n_query, const int64_t* uptr, const int32_t* hist, int k,
                     int32_t* out_idx, float* out_score, void* ws, size_t ws_bytes, hipStream_t st);

// fusion MLP (ppgat_fusion.hip)
bool fusion_shape_ok(int Dt, int Di, int h1, int d_out);
size_t fusion_workspace_bytes(int Dt, int Di);
hipError_t fusion_fwd(const float* txt, const float* img, const int32_t* img_index, const float* img_fallback,
                      int64_t B, int Dt, int Di, const float* W1, const float* b1, const float* W2, const float* b2,
                      int normalize, float* out, float* z1_out, hipStream_t st,
                      void* ws = nullptr);

// index-range validation (ppgat_debug.hip)
hipError_t count_out_of_range(const void* idx, int elem_bytes, int64_t n, int64_t lo, int64_t hi, int64_t* n_bad,
                              hipStream_t st);

// fusion MLP training: InfoNCE loss + backward, ReLU/dropout (ppgat_infonce.hip)
bool infonce_shape_ok(int64_t B, int D);
size_t infonce_workspace_bytes(int64_t B);
hipError_t infonce(const float* F, const float* T, const float* I, int64_t B, float tau, float* loss, float* dF,
                   float* dT, float* dI, void* ws, hipStream_t st);
hipError_t relu_dropout(const float* z, int64_t n, float p, uint64_t seed, int backward, float* a, hipStream_t st);

// matrix-core GEMMs (ppgat_xform.hip) and the aggregate-then-transform multi-head layer
// (ppgat_xgat.hip: att_proj, rank_update, xgat_*, colsum)
hipError_t seed_snapshot(uint64_t seed, uint64_t* out, hipStream_t st);
bool gemm_nn_shape_ok(int64_t M, int K, int N, int bmode);
// split-bf16 matrix-core GEMMs on (default) or the fp32 MFMA kernels (PPGAT_GEMM=fp32)
bool gemm_split_enabled();
hipError_t gemm_nn(const float* X, int64_t ldx, int64_t M, int K, const float* B, int64_t ldb, int bmode, int N,
                   float alpha, const float* bias, float* Y, int64_t ldy, hipStream_t st,
                   void* ws = nullptr, const float* rS = nullptr, int64_t ldrs = 0, int nv = 0,
                   const float* rA = nullptr, int64_t ldra = 0);
size_t gemm_nn_workspace_bytes(int64_t M, int K, int N);
// bytes of the split bf16 images of a GEMM's B operand per (32 nt columns, 32-deep k chunk)
size_t nnx_image_bytes(int K, int N, int nt);
// the fp16 two-term family: pre-split images + column exponents
size_t nnh_image_bytes(int K, int N, int nt);
hipError_t nnh_presplit(const float* B, int64_t ldb, int bmode, int K, int N, int nt, uint16_t* img, int* ecol,
                        hipStream_t st);
// A [2H, K] = [W_h^T att_src[h]; W_h^T att_dst[h]] (any shape) and dx += S A (rank nv <= 16)
hipError_t att_proj(const float* W, const float* att_src, const float* att_dst, int H, int C, int K, float* A,
                    hipStream_t st);
hipError_t rank_update(const float* S, int64_t lds, int nv, const float* A, int64_t lda, int64_t n, int K, float* dx,
                       int64_t lddx, hipStream_t st);
bool gemm_tn_big_shape_ok(int Ma, int Nb);
size_t gemm_tn_big_workspace_bytes(int64_t M, int Ma, int Nb);
hipError_t gemm_tn_big(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t M, int Ma, int Nb, float* out,
                       void* ws, hipStream_t st, const unsigned* b_bound = nullptr, int b_period = 0,
                       float b_scale = 1.f, const unsigned* a_bound = nullptr, float* colsum_out = nullptr);
hipError_t colmax_abs(const float* X, int64_t ldx, int64_t M, int C, unsigned* out, hipStream_t st,
                      const int32_t* src_ptr = nullptr);
bool xgat_shape_ok(int K, int H, int C);
hipError_t xgat_weights(const float* W, const float* att_src, const float* att_dst, int H, int C, int K, float* A,
                        float* Wt, float* Wg, hipStream_t st);
hipError_t xgat_scores(const float* x, int64_t ldx, int64_t n_rows, int64_t n_dst, int K, int H, const float* A,
                       float* s_src, float* s_dst, hipStream_t st);
hipError_t xgat_fwd(const ppgat_schedule& sch, const int32_t* col, const int32_t* eid, const float* x, int64_t ldx,
                    int K, int H, const float* s_src, const float* s_dst, float slope, float p, uint64_t seed,
                    const uint64_t* seed_in, float* agg, float* m, float* invl, float* partial, hipStream_t st,
                    unsigned* xmax = nullptr);
hipError_t xgat_bwd_pro(const float* gt, const float* agg, const float* s_dst, const float* m, const float* invl,
                        int64_t n, int K, int H, float* nstate, hipStream_t st);
hipError_t xgat_bwd_edges(const ppgat_schedule& sch, const int32_t* row, const int32_t* csc_eid,
                          const int32_t* csc2csr,
                          const float* x, int64_t ldx, int K, int H, const float* s_src, const float* nstate,
                          const float* gt, const float* A_src, float slope, float p, uint64_t seed,
                          const uint64_t* seed_in, float* dx, int64_t lddx, float* S, int64_t lds, float* dz,
                          float* partial, hipStream_t st);
hipError_t xgat_bwd_edges_g(const ppgat_schedule& sch, const int32_t* row, const int32_t* csc_eid,
                            const int32_t* csc2csr,
                            const float* hs, int C, int H, const float* s_src, const float* nstate, const float* g,
                            int64_t ldg, float slope, float p, uint64_t seed, const uint64_t* seed_in, float* acc,
                            float* S, int64_t lds, float* dz, float* partial, hipStream_t st, float* pz = nullptr,
                            unsigned* gmax = nullptr);
hipError_t xgat_nstate_set_d(float* nstate, const float* D, int64_t n, int H, hipStream_t st);
hipError_t xgat_nstate(const float* s_dst, const float* m, const float* invl, const float* D, int64_t n, int H,
                       float* nstate, hipStream_t st);
hipError_t xgat_bwd_dz(const ppgat_schedule& sch, const int32_t* row, const int32_t* csc_eid, const int32_t* csc2csr,
                       int H,
                       const float* s_src, const float* nstate, float slope, float p, uint64_t seed,
                       const uint64_t* seed_in, float* dz, float* S, int64_t lds, float* partial, hipStream_t st);
hipError_t xgat_bwd_epi(const float* S, int64_t lds, const float* A_dst, int64_t n, int K, int H, float* dx,
                        int64_t lddx, hipStream_t st);
hipError_t xgat_wgrad(const float* G, const float* GV, const float* W, const float* att_src, const float* att_dst,
                      int H, int C, int K, float* dW, float* datt_src, float* datt_dst, hipStream_t st);
int64_t colsum_blocks(int64_t n);
hipError_t colsum(const float* Y, int64_t ldy, int64_t n, int C, float* out, float* part, hipStream_t st);

}  // namespace ppgat
