/*
 * ppgat.h -- C ABI of the MI355X-native GAT message-passing library (libppgat.so).
 *
 * This is the drop-in boundary beneath the reference's GAT layer call site
 *     x = conv(x, edge_index)          scripts/train_gat_pyg.py:86-87
 *     x = gat(x, edge_index)           scripts/train_gat_custom.py:113-114
 * i.e. torch_geometric.nn.GATConv(hidden, hidden, heads=H, dropout=p,
 * add_self_loops=False, concat=False)  (scripts/train_gat_pyg.py:77) and
 * SimpleGATLayer.forward               (scripts/train_gat_custom.py:75-93).
 *
 * Conventions
 *  - every pointer is DEVICE memory allocated by the caller (the library never
 *    allocates or frees device memory; workspace sizes are queried first);
 *  - float tensors are fp32, row-major, contiguous; node rows are [N, H, C];
 *  - indices are int32 after preprocessing (edge_index stays int64 on input);
 *  - work is enqueued on `stream` (a hipStream_t passed as void*); no host sync
 *    except where a function says so;
 *  - return 0 on success, nonzero on error; ppgat_last_error() gives a
 *    thread-local message.  Unsupported shapes return PPGAT_ERR_UNSUPPORTED.
 *
 * Semantics (mode):
 *  PPGAT_MODE_PYG    : e = leaky_relu(s_src[j] + s_dst[i], slope);
 *                      alpha = exp(e - max_i) / (sum exp(e - max_i) + 1e-16);
 *                      out_i = mean_h sum_j alpha * h_j + bias    (PyG GATConv, concat=False)
 *  PPGAT_MODE_CUSTOM : e = clamp(leaky_relu(z, 0.2), -10, 10); alpha = exp(e) / (sum exp(e) + 1e-9);
 *                      out_i = sum_j alpha * h_j        (SimpleGATLayer, heads must be 1, bias NULL)
 *  Dropout on alpha (training) uses a counter-based hash of (seed, original edge id, head):
 *  keep iff u(seed, eid, head) >= p, kept values scaled by 1/(1-p).  The same mask is
 *  regenerated in the backward pass and restated bit-for-bit in oracle/gat_oracle.py.
 */
#ifndef PPGAT_H
#define PPGAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPGAT_OK 0
#define PPGAT_ERR_INVALID 1
#define PPGAT_ERR_UNSUPPORTED 2
#define PPGAT_ERR_HIP 3

#define PPGAT_MODE_PYG 0
#define PPGAT_MODE_CUSTOM 1

/* Library identification: 2 = ppgat_schedule carries n_long_items (schedule counts int32[4]);
 * 3 = ppgat_fwd / ppgat_bwd / ppgat_bwd_edges carry seed_used, ppgat_adam_step_device takes one
 * step pointer per tensor. */
int ppgat_version(void);
const char* ppgat_last_error(void);

/* Channels per head the fused kernels are instantiated for (C in {4,8,...,256}). */
int ppgat_supported_channels(int channels);

/* ---- graph preprocessing ------------------------------------------------
 * Replaces: the COO edge_index consumed by GATConv.propagate / index_add_
 * (scripts/train_gat_pyg.py:139-147 builds it; train_gat_custom.py:78,86-92 uses it).
 * Builds, from edge_index int64 [2,E] (row 0 = src, row 1 = dst):
 *   CSR by destination : rowptr[N+1], col[E] (= src), csr_eid[E] (original column id)
 *   CSC by source      : colptr[N+1], row[E] (= dst), csc_eid[E], csc2csr[E] (CSR slot of each CSC edge)
 * In-segment order is the original column order (stable), so results are deterministic.
 * bad_count (device int32[1]) receives the number of out-of-range indices (0 = valid).
 */
int ppgat_csr_workspace_bytes(int64_t n_nodes, int64_t n_edges, size_t* bytes);
int ppgat_csr_build(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes,
                    int32_t* rowptr, int32_t* col, int32_t* csr_eid,
                    int32_t* colptr, int32_t* row, int32_t* csc_eid, int32_t* csc2csr,
                    int32_t* bad_count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- work schedule -------------------------------------------------------
 * Cuts the rows of a CSR/CSC (ptr[N+1]) into work items of at most max_edges edges for
 * the fused kernels: rows with deg > max_edges ("hubs") become ceil(deg/max_edges)
 * pieces listed first (hubs in row order, pieces merged deterministically afterwards),
 * then every other row as one item in descending-degree order (longest work first).
 * Capacities: items <= ppgat_schedule_capacity(), hub_row <= N, hub_ptr <= N+1.
 * counts (device int32[4]) receives {n_hubs, n_hub_items, n_items, n_long_rows}, n_long_rows
 * = rows that are not hubs and have more than PPGAT_SHORT_ITEM_EDGES edges; the caller
 * reads it once (a one-time host sync per static graph) to fill a ppgat_schedule, with
 * n_long_items = n_hub_items + n_long_rows.
 */
#define PPGAT_SHORT_ITEM_EDGES 16
typedef struct ppgat_schedule {
  const int32_t* item_row;  /* [n_items] row (dst for CSR, src for CSC) */
  const int32_t* item_beg;  /* [n_items] first edge slot */
  const int32_t* item_end;  /* [n_items] one past the last edge slot */
  int64_t n_items;
  int64_t n_hub_items;      /* items [0, n_hub_items) are hub pieces */
  const int32_t* hub_row;   /* [n_hubs] */
  const int32_t* hub_ptr;   /* [n_hubs+1] piece (= item) ranges per hub */
  int64_t n_hubs;
  int64_t n_long_items;     /* items [0, n_long_items) have > PPGAT_SHORT_ITEM_EDGES edges; the
                               rest (descending degree) are run four per wavefront (heads = 1).
                               -1: unknown (every item takes the one-per-wavefront path) */
} ppgat_schedule;

int64_t ppgat_schedule_capacity(int64_t n_nodes, int64_t n_edges, int32_t max_edges);
int ppgat_schedule_workspace_bytes(int64_t n_nodes, size_t* bytes);
int ppgat_schedule_build(const int32_t* ptr, int64_t n_nodes, int64_t n_edges, int32_t max_edges,
                         int32_t* item_row, int32_t* item_beg, int32_t* item_end,
                         int32_t* hub_row, int32_t* hub_ptr, int32_t* counts,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-node attention terms -------------------------------------------
 * Replaces: PyG alpha_src = (x * att_src).sum(-1), alpha_dst likewise (GATConv.forward);
 *           custom (h[src]*a_src).sum(-1) / (h[dst]*a_dst).sum(-1) (train_gat_custom.py:79),
 *           hoisted from edges to nodes.
 * h [N,H,C], att_src/att_dst [H,C] -> s_src/s_dst [N,H].
 */
int ppgat_node_scores(const float* h, const float* att_src, const float* att_dst,
                      int64_t n_nodes, int heads, int channels,
                      float* s_src, float* s_dst, void* stream);

/* ---- fused forward -------------------------------------------------------
 * Replaces: GATConv edge_update + softmax + dropout + propagate/SumAggregation + head mean + bias
 *           (train_gat_pyg.py:77,87 -> PyG), and train_gat_custom.py:78-93.
 * dst_sched: schedule over the CSR by destination (rowptr).  Writes out [N,C], the
 * per-(node,head) softmax state m [N,H] and inv_l = 1/(l+eps) [N,H] (saved for the
 * backward), and agg [N,H,C] (per-head aggregate) when agg != NULL (required for heads > 1
 * training).  workspace: hub-piece partials, ppgat_fwd_workspace_bytes().
 * seed_used (device uint64[1], nullable; written when dropout_p > 0): the effective mask seed
 * (seed folded with the dropout epoch at the time the forward runs).  Passing it to the
 * backward below makes the backward regenerate exactly the forward's mask even if the epoch
 * advances in between (ppgat_dropout_advance from another replayed graph, a recompute).
 */
int ppgat_fwd_workspace_bytes(int64_t n_hub_items, int heads, int channels, size_t* bytes);
int ppgat_fwd(const ppgat_schedule* dst_sched, const int32_t* col, const int32_t* csr_eid,
              int64_t n_nodes, int64_t n_edges, int heads, int channels,
              const float* h, const float* s_src, const float* s_dst, const float* bias,
              int mode, float negative_slope, float dropout_p, uint64_t seed, uint64_t* seed_used,
              float* out, float* m, float* inv_l, float* agg,
              void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused backward ------------------------------------------------------
 * Replaces: autograd of the ops above (index_put_ accumulate, mul backward, scatter
 *           backward; 34%+25%+11.5% of the reference CPU step).
 * src_sched: schedule over the CSC by source (colptr).  Given grad_out [N,C] returns
 * grad_h [N,H,C] (message term plus the attention-logit terms ds_src (x) att_src +
 * ds_dst (x) att_dst), grad_att_src/grad_att_dst [H,C] and, when grad_bias != NULL,
 * grad_bias [C] = column sums of grad_out.  Atomic-free and
 * deterministic (segment-owned sums in a fixed order).  agg may be NULL when heads == 1
 * (out - bias is used).  seed_used: the forward's ppgat_fwd seed_used (nullable: then seed is
 * folded with the current dropout epoch).
 */
int ppgat_bwd_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_hub_items, int heads, int channels,
                              size_t* bytes);
int ppgat_bwd(const ppgat_schedule* src_sched, const int32_t* rowptr, const int32_t* row,
              const int32_t* csc_eid, const int32_t* csc2csr,
              int64_t n_nodes, int64_t n_edges, int heads, int channels,
              const float* h, const float* s_src, const float* s_dst,
              const float* att_src, const float* att_dst, const float* bias,
              const float* out, const float* agg, const float* m, const float* inv_l,
              const float* grad_out,
              int mode, float negative_slope, float dropout_p, uint64_t seed, const uint64_t* seed_used,
              float* grad_h, float* grad_att_src, float* grad_att_dst, float* grad_bias,
              void* workspace, size_t workspace_bytes, void* stream);

/* ---- backward, staged (multi-GPU: collectives go between the stages) ----------
 * ppgat_bwd == prologue -> edges -> epilogue on one device.  Row-sharded:
 *  prologue over the rank's own destination rows -> nstate (all-gathered with grad_out),
 *  edges over the rank's own SOURCE rows (CSC slice; `row` indexes the gathered dst space,
 *  dz_slot gives each edge's position in a [world x max-local-edges] dz buffer that is then
 *  reduce-scattered), epilogue over the own destination rows with the local dz.
 *  dz_slot == NULL: each edge's dz goes to its own CSC position (read back through
 *  ppgat_bwd_dst_sum_csc); csc2csr as dz_slot gives the CSR-order layout of ppgat_bwd_dst_sum.
 *  nstate: [N_dst, H] float4 {s_dst, m, inv_l, D}.  grad_bias (nullable) needs bias_part
 *  [ppgat_bwd_partial_rows(n) * C]; epilogue part: [ppgat_bwd_partial_rows(n) * 2*H*C].
 *
 * Zero-row mark.  D with the bit pattern 0x80000000 (-0.0f) means "this destination's grad_out
 * row is all zeros".  ppgat_bwd_prologue writes it exactly for those rows and +0.0f for any other
 * D that is zero; so do the fused producers (ppgat_bpr_bwd_producer: the rows no triple names;
 * ppgat_project_bwd_fused_producer never marks).  A caller that builds nstate itself must not
 * store -0.0f in D for a row whose grad_out is not all zeros.
 *
 * Gather skipping (ppgat_set_gather_skip, default on).  ppgat_fwd / ppgat_edge_fwd do not load
 * h_j of an edge whose weight exp(e - m) * dropout is exactly 0; ppgat_bwd_edges /
 * ppgat_edge_bwd_edges (heads = 1, and the per-head kernel taken when heads is not 2, 4 or 8 or
 * C < 32) do not load grad_out row i of an edge with beta = c1 = 0 (a dropped edge) or whose
 * destination carries the zero-row mark.  The skipped terms are exact zeros, so every output
 * equals the unskipped one, with two exceptions:
 *  - a non-finite value in a row reached only through such edges no longer makes the result NaN
 *    (0 x NaN is not computed);
 *  - dz of a dropped edge whose c0 is exactly 0 may be +0 where it was -0 or the reverse.
 * The multi-head pass (heads 2, 4, 8), the aggregate-then-transform and the GATv2 kernels gather
 * every row.  Returns the previous value; read by each launch, so a captured graph keeps the
 * value it was captured with.  The Python package applies PPGAT_GATHER_SKIP=0 once, when it
 * loads the library (the library itself does not read the environment).
 */
int ppgat_set_gather_skip(int on);
int64_t ppgat_bwd_partial_rows(int64_t n_nodes);
int ppgat_bwd_prologue(const float* grad_out, const float* out, const float* agg, const float* bias,
                       const float* s_dst, const float* m, const float* inv_l, int64_t n_nodes, int heads,
                       int channels, int mode, float* nstate, float* grad_bias, float* bias_part, void* stream);
int ppgat_bwd_edges(const ppgat_schedule* src_sched, const int32_t* row, const int32_t* csc_eid,
                    const int32_t* dz_slot, int64_t n_edges, int heads, int channels, const float* h,
                    const float* s_src, const float* nstate, const float* grad_out, int mode, float negative_slope,
                    float dropout_p, uint64_t seed, const uint64_t* seed_used, float* grad_h, int64_t ld_grad_h,
                    float* ds_src,
                    int64_t ld_ds_src, float* dz, void* workspace, size_t workspace_bytes, void* stream);
/* ds_dst[i*ld + h] = sum of dz over the CSR segment of destination i, walked with the
 * forward (destination) schedule so hub rows are split; workspace >= n_hub_items*heads*4
 * bytes (hub partials, added in piece order: deterministic).  With
 * grad_h and ds_src/ds_dst written side by side into one [N, ld] buffer
 * D = [dh_msg | ds_src | ds_dst], the projection gradients follow from two GEMMs with
 * W_aug = [W; A_src; A_dst] (A_src[h] = sum_c att_src[h,c] W[h*C+c, :]):
 *   dx = D W_aug,   D^T x = [dh_msg^T x ; ds_src^T x ; ds_dst^T x]  (ppgat_gemm_tn with V),
 *   dW = dh_msg^T x + att_src (x) (ds_src^T x) + att_dst (x) (ds_dst^T x),
 *   datt_src[h] = W_h (ds_src^T x)[h],  datt_dst[h] = W_h (ds_dst^T x)[h]. */
int ppgat_bwd_dst_sum(const ppgat_schedule* fwd_sched, int64_t n_nodes, int heads, const float* dz, float* ds_dst,
                      int64_t ld_ds_dst, void* workspace, size_t workspace_bytes, void* stream);
/* Same sums with dz in CSC (source) order -- the layout ppgat_bwd_edges writes when dz_slot is
 * NULL (contiguous per-edge stores instead of a 4-B scatter per edge): CSR slot k of a
 * destination reads dz[csr2csc[k]], csr2csc = the inverse of ppgat_csr_build's csc2csr
 * (ppgat_invert_index).  Same summation order, so the result equals ppgat_bwd_dst_sum's on the
 * CSR-order layout bit for bit. */
int ppgat_bwd_dst_sum_csc(const ppgat_schedule* fwd_sched, int64_t n_nodes, int64_t n_edges, int heads,
                          const float* dz, const int32_t* csr2csc, float* ds_dst, int64_t ld_ds_dst,
                          void* workspace, size_t workspace_bytes, void* stream);
/* inverse[index[k]] = k for a permutation index of [0, n) (int32). */
int ppgat_invert_index(const int32_t* index, int64_t n, int32_t* inverse, void* stream);
int ppgat_bwd_epilogue(const int32_t* rowptr, int64_t n_nodes, int heads, int channels, const float* h,
                       const float* att_src, const float* att_dst, const float* ds_src, const float* dz,
                       float* grad_h, float* grad_att_src, float* grad_att_dst, float* part, void* stream);

/* ---- GATConv edge features (edge_dim = D) ----------------------------------
 * Replaces: PyG GATConv(edge_dim=D): alpha_edge = (lin_edge(edge_attr).view(E, H, C) * att_edge).sum(-1)
 *           added to the logit before leaky_relu.  The caller collapses the two parameters to
 *           v [H, D], v[h, d] = sum_c att_edge[h, c] lin_edge.weight[h C + c, d]; then
 *           alpha_edge[k, h] = <edge_attr[k, :], v[h, :]>.  D <= PPGAT_EDGE_MAX_DIM, heads <= 8.
 * ppgat_edge_attr_permute: out[k, :] = edge_attr[slot_eid[k], :] -- edge_attr [E, D] brought into
 *   the slot order of a view (slot_eid = csr_eid or csc_eid of ppgat_csr_build), once per graph
 *   and attribute tensor.
 * ppgat_edge_terms: t_csr[k, h] = <attr_csr[k, :], v[h, :]> and (t_csc != NULL) t_csc likewise
 *   from attr_csc: the same fmaf chain over d for both, so an edge's term has the same bits in
 *   either order.
 * ppgat_edge_fwd / ppgat_edge_bwd_edges: ppgat_fwd / ppgat_bwd_edges with the logit
 *   z = (s_src[j] + s_dst[i]) + edge_term[k, h] -- edge_term [E, H] in CSR slot order for the
 *   forward, in CSC slot order for pass B.  Everything else as documented above.
 * ppgat_edge_dv: dv[h, d] = sum_k dz[k, h] attr_csc[k, d] with dz [E, H] in CSC order (pass B
 *   with dz_slot NULL).  A fixed grid leaves one partial row per block in part
 *   [ppgat_edge_dv_partial_rows(E) * H * D], summed in block order: atomic-free, the same bits on
 *   every launch.  E = 0 gives dv = 0.
 */
#define PPGAT_EDGE_MAX_DIM 16
int ppgat_edge_attr_permute(const float* edge_attr, const int32_t* slot_eid, int64_t n_edges, int edge_dim,
                            float* out, void* stream);
int ppgat_edge_terms(const float* attr_csr, const float* attr_csc, const float* v, int64_t n_edges, int edge_dim,
                     int heads, float* t_csr, float* t_csc, void* stream);
int ppgat_edge_fwd(const ppgat_schedule* dst_sched, const int32_t* col, const int32_t* csr_eid,
                   const float* edge_term, int64_t n_nodes, int64_t n_edges, int heads, int channels,
                   const float* h, const float* s_src, const float* s_dst, const float* bias,
                   int mode, float negative_slope, float dropout_p, uint64_t seed, uint64_t* seed_used,
                   float* out, float* m, float* inv_l, float* agg,
                   void* workspace, size_t workspace_bytes, void* stream);
int ppgat_edge_bwd_edges(const ppgat_schedule* src_sched, const int32_t* row, const int32_t* csc_eid,
                         const int32_t* dz_slot, const float* edge_term, int64_t n_edges, int heads, int channels,
                         const float* h, const float* s_src, const float* nstate, const float* grad_out, int mode,
                         float negative_slope, float dropout_p, uint64_t seed, const uint64_t* seed_used,
                         float* grad_h, int64_t ld_grad_h, float* ds_src, int64_t ld_ds_src, float* dz,
                         void* workspace, size_t workspace_bytes, void* stream);
int64_t ppgat_edge_dv_partial_rows(int64_t n_edges);
int ppgat_edge_dv(const float* dz, const float* attr_csc, int64_t n_edges, int heads, int edge_dim, float* dv,
                  float* part, void* stream);

/* ---- loss of the training step ---------------------------------------------
 * Replaces: pos = (U[u]*I[i]).sum(-1); neg = (U[u]*I[j]).sum(-1); BPR
 *           -log(sigmoid(pos-neg)+1e-8).mean() (loss_kind 0) or BCE-with-logits over
 *           [pos; neg] with labels [1; 0] (loss_kind 1)  -- scripts/train_gat_pyg.py:313-322,
 *           and its autograd (gather backward = index_put_ accumulate).
 * Z [n_rows, C]; node id v (users [0, n_users), items n_users + i) lives in row v, or in
 * row row_map[v] when row_map != NULL (int32 [n_users + n_items]; the row-sharded path keeps
 * the gathered Z in a padded per-rank layout).  A user whose row_map entry is -1 is not held
 * by this caller: its triples contribute nothing (loss 0, no gradient), while the mean still
 * divides by S -- the row-sharded loss evaluates the triples of its own users only and
 * the ranks' losses add up to the reference's.  u, i, j int64 [S].
 * Forward writes the scalar mean loss and coef [S, 2] (dloss/dpos, dloss/dneg); the
 * backward writes the full grad_Z [N, C] (zero rows included) = grad_loss * sum of the
 * per-triple contributions, deterministically (sorted contributions, ordered sums).
 * Indices outside their range are clamped and counted into bad_count (device int32[1],
 * nullable; zeroed by the call) so the caller can raise without a host sync here.
 */
int ppgat_bpr_workspace_bytes(int64_t n_rows, int64_t n_samples, int channels, size_t* bytes);
int ppgat_bpr_fwd(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, const int32_t* row_map,
                  int channels, const int64_t* u, const int64_t* i, const int64_t* j, int64_t n_samples,
                  int loss_kind, float* loss, float* coef, int32_t* bad_count, void* workspace,
                  size_t workspace_bytes, void* stream);
int ppgat_bpr_bwd(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, const int32_t* row_map,
                  int channels, const int64_t* u, const int64_t* i, const int64_t* j, int64_t n_samples,
                  const float* coef, const float* grad_loss, float* grad_Z,
                  void* workspace, size_t workspace_bytes, void* stream);
/* ppgat_bpr_bwd in two calls: the part that depends on the triples only (their destination
 * rows, sorted; the touched-row marks) and the rest.  The first may run on another stream while
 * the model computes Z (train_gat_pyg.py:313-322 samples the triples before the forward); the
 * second must be stream-ordered after it and after ppgat_bpr_fwd, on the same workspace, with
 * the same sizes, row_map and u, i, j.  Same result as ppgat_bpr_bwd, bit for bit. */
int ppgat_bpr_bwd_prepare(int64_t n_rows, int64_t n_users, int64_t n_items, const int32_t* row_map, int channels,
                          const int64_t* u, const int64_t* i, const int64_t* j, int64_t n_samples,
                          void* workspace, size_t workspace_bytes, void* stream);
int ppgat_bpr_bwd_prepared(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, const int32_t* row_map,
                           int channels, const int64_t* u, const int64_t* i, const int64_t* j, int64_t n_samples,
                           const float* coef, const float* grad_loss, float* grad_Z,
                           void* workspace, size_t workspace_bytes, void* stream);
/* ppgat_bpr_bwd (row_map NULL, after ppgat_bpr_fwd on the same workspace) that also does the
 * backward prologue of the GAT layer whose output Z is (heads = 1; the last conv of
 * train_gat_pyg.py:86-87 feeding the loss of :313-322) -- ppgat_bwd_prologue's outputs for that
 * layer from grad_Z while its rows are on chip, instead of a second pass over grad_Z and Z:
 *   prev_nstate[r] = {prev_s_dst[r], prev_m[r], prev_inv_l[r], prev_gscale <dZ_r, Z_r - prev_bias>}
 *   prev_grad_bias = sum_r dZ_r                    (prev_bias / prev_grad_bias nullable)
 * Z_r is loaded with the row's last contributions, so the dot adds no round trip.  grad_Z bit
 * for bit that of ppgat_bpr_bwd; deterministic. */
int ppgat_bpr_bwd_producer(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, int channels,
                           const int64_t* u, const int64_t* i, const int64_t* j, int64_t n_samples, const float* coef,
                           const float* grad_loss, float* grad_Z, const float* prev_bias, const float* prev_s_dst,
                           const float* prev_m, const float* prev_inv_l, float prev_gscale, float* prev_nstate,
                           float* prev_grad_bias, void* workspace, size_t workspace_bytes, void* stream);

/* ---- sampled-softmax loss: one positive against M sampled negatives -----------
 * Replaces: nothing one-to-one -- the reference trains on one negative per positive
 *           (scripts/train_gat_pyg.py:313-322).  In torch terms, with cand [S, M + 1] (column 0
 *           the positive, e.g. from ppgat_eval_sample):
 *             s = (Z[u][:, None, :] * Z[n_users + cand]).sum(-1) / temperature
 *             loss = (s.logsumexp(1) - s[:, 0]).mean()
 *           and its autograd (index_select backward = index_add_ with float atomics).
 * Z [n_rows, C] with n_rows = n_users + n_items; u int64 [S]; cand int64 [S, n_cand], n_cand =
 * M + 1 >= 2.  A candidate may repeat in a row and the positive may appear among the negatives:
 * both simply add terms.  The forward writes the scalar mean loss and coef [S, n_cand] =
 * (softmax - [m == 0]) / (S temperature); the backward writes every row of grad_Z [n_rows, C]
 * exactly once (zero rows included) = grad_loss (a device scalar) times the sums of the
 * contributions, without float atomics: sorted records, ordered sums, the same bits on every
 * launch.  n_samples == 0: loss 0, zero gradient.  Indices outside their range are clamped and
 * counted into bad_count (device int32[1], nullable; written by the call).  Both calls take the
 * workspace of the first function (host only); the backward needs nothing the forward left in it.
 */
int ppgat_ssm_workspace_bytes(int64_t n_rows, int64_t n_samples, int64_t n_cand, int channels, size_t* bytes);
int ppgat_ssm_fwd(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, int channels, const int64_t* u,
                  const int64_t* cand, int64_t n_samples, int64_t n_cand, float temperature, float* loss, float* coef,
                  int32_t* bad_count, void* workspace, size_t workspace_bytes, void* stream);
int ppgat_ssm_bwd(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, int channels, const int64_t* u,
                  const int64_t* cand, int64_t n_samples, int64_t n_cand, float temperature, const float* coef,
                  const float* grad_loss, float* grad_Z, void* workspace, size_t workspace_bytes, void* stream);
/* The forward with a sampling correction (logQ): corr fp32 [n_items], finite, is subtracted from
 * the logit of every negative, s[t, m] -= corr[cand[t, m]] for m >= 1, never from the
 * positive's, before the online maximum is taken.  It carries no gradient, so coef is the
 * softmax of the corrected logits and ppgat_ssm_bwd is the backward of this forward too. */
int ppgat_ssm_fwd_corrected(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, int channels,
                            const int64_t* u, const int64_t* cand, const float* corr, int64_t n_samples,
                            int64_t n_cand, float temperature, float* loss, float* coef, int32_t* bad_count,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- shared-negatives softmax loss: one pool of P items scored against every positive ----
 * Replaces: nothing one-to-one -- the reference trains on one negative per positive
 *           (scripts/train_gat_pyg.py:313-322).  In torch terms, with pool [P] ascending item ids
 *           and hit [S, P] = (pool[None, :] == pos[:, None]) | (pool[j] in history(u[t])):
 *             U = Z[u];  s0 = (U * Z[n_users + pos]).sum(-1) / temperature
 *             s = (U @ Z[n_users + pool].T / temperature).masked_fill(hit, -inf)
 *             loss = (torch.cat([s0[:, None], s], 1).logsumexp(1) - s0).mean()
 *           and its autograd (matmul backward plus index_add_ with float atomics).
 * Z [n_rows, C] with n_rows = n_users + n_items; u, pos int64 [S]; pool int64 [P], P >= 1,
 * strictly ascending (so distinct).  hist_ptr int64 [n_users + 1] and hist_items int32, sorted
 * per user (the sampler's arrays, as ppgat_full_rank takes them), nullable together: without them
 * only a sample's own positive is masked.  The [S, P] scores are a split-bf16 matrix-core
 * product at fp32 accuracy and are never written.  The forward writes the scalar mean loss,
 * lse [S] and c0 [S] = (p0 - 1) / (S temperature), formed without cancellation, and leaves the
 * mask words [S, ceil(P / 32)] in the workspace: the backward takes the SAME workspace,
 * untouched since the forward.  A sample whose whole pool is masked has loss term 0 and c0 = 0.
 * The backward recomputes the scores from Z and lse and writes every row of grad_Z [n_rows, C]
 * (zero rows included) = grad_loss (a device scalar) times the sums of the contributions, without
 * float atomics and in a fixed order: the same bits on every launch.  n_samples == 0: loss 0,
 * zero gradient.  Indices outside their range are clamped and counted into bad_count[0]; pool
 * entries not above their predecessor are counted into bad_count[1] (device int32[2], written
 * by the forward).  channels in {64, 128} (ppgat_shs_supported); others: PPGAT_ERR_UNSUPPORTED
 * before any device work.  Workspace (host only): O(S C + P C + S P / 8) bytes.
 */
int ppgat_shs_supported(int channels);
int ppgat_shs_workspace_bytes(int64_t n_rows, int64_t n_samples, int64_t n_pool, int channels, size_t* bytes);
int ppgat_shs_fwd(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, int channels, const int64_t* u,
                  const int64_t* pos, int64_t n_samples, const int64_t* pool, int64_t n_pool,
                  const int64_t* hist_ptr, const int32_t* hist_items, float temperature, float* loss, float* lse,
                  float* c0, int32_t* bad_count, void* workspace, size_t workspace_bytes, void* stream);
int ppgat_shs_bwd(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, int channels, const int64_t* u,
                  const int64_t* pos, int64_t n_samples, const int64_t* pool, int64_t n_pool, float temperature,
                  const float* lse, const float* c0, const float* grad_loss, float* grad_Z, void* workspace,
                  size_t workspace_bytes, void* stream);
/* The pair with a sampling correction (logQ): corr fp32 [n_items], finite, is subtracted from
 * every pool logit, s[t, j] -= corr[pool[j]], never from the positive's s0.  corr[pool] is
 * gathered once by the forward into its workspace (that of the _corrected size function, which
 * the backward takes untouched, as above) and applied to the accumulator in the forward and in
 * both backward sweeps in one association order, so the backward recomputes the forward's bits.
 * No gradient flows to corr.  Everything else is as for the uncorrected pair. */
int ppgat_shs_corrected_workspace_bytes(int64_t n_rows, int64_t n_samples, int64_t n_pool, int channels,
                                        size_t* bytes);
int ppgat_shs_fwd_corrected(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, int channels,
                            const int64_t* u, const int64_t* pos, int64_t n_samples, const int64_t* pool,
                            int64_t n_pool, const int64_t* hist_ptr, const int32_t* hist_items, const float* corr,
                            float temperature, float* loss, float* lse, float* c0, int32_t* bad_count,
                            void* workspace, size_t workspace_bytes, void* stream);
int ppgat_shs_bwd_corrected(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, int channels,
                            const int64_t* u, const int64_t* pos, int64_t n_samples, const int64_t* pool,
                            int64_t n_pool, float temperature, const float* lse, const float* c0,
                            const float* grad_loss, float* grad_Z, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ---- projection weight gradient ----------------------------------------------
 * Replaces: the weight (and bias) gradient of torch.nn.Linear in GATConv.lin /
 *           SimpleGATLayer.lin (train_gat_custom.py:66,77) and PyGGAT.item_proj
 *           (train_gat_pyg.py:74,81): out[M,K] = A[N,M]^T B[N,K]; colsum[M] = sum_n A[n,:]
 *           when colsum != NULL; vout[nv, K] = V[N, nv]^T B when nv > 0 (nv <= 16).
 *           Row strides lda/ldb/ldv (floats; lda, ldb multiples of 4).  fp32 in, fp32 MFMA
 *           (exact fp32 FMA), N split over workgroups with an ordered reduction of the
 *           partials (deterministic).
 */
int ppgat_gemm_tn_workspace_bytes(int64_t n, int m, int k, int nv, size_t* bytes);
int ppgat_gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n, int m, int k, float* out,
                  float* colsum, const float* V, int64_t ldv, int nv, float* vout,
                  void* workspace, size_t workspace_bytes, void* stream);

/* Same as ppgat_gemm_tn with B given as two row segments: rows [0, split) from b0 (ldb0),
 * rows [split, n) from b1 (row - split, ldb1) -- x = cat(user_emb, item_proj(feats))
 * (train_gat_pyg.py:79-82) without materialising the concatenation. */
int ppgat_gemm_tn_seg(const float* A, int64_t lda, const float* b0, int64_t ldb0, const float* b1, int64_t ldb1,
                      int64_t split, int64_t n, int m, int k, float* out, float* colsum, const float* V, int64_t ldv,
                      int nv, float* vout, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused projection (matrix cores) ------------------------------------------------
 * Replaces: h = GATConv.lin(x) (PyG Linear, no bias; train_gat_pyg.py:77) /
 *           SimpleGATLayer.lin (train_gat_custom.py:66,77) followed by the node attention
 *           terms (alpha_src/alpha_dst; custom :79), and PyGGAT.item_proj (train_gat_pyg.py:74,81):
 *   y[r, :] = x_r W^T (+ bias),   x_r = x0[r] for r < split, x1[r - split] otherwise
 *   s_src[r] = y[r] . att_src,  s_dst[r] = y[r] . att_dst   when att_src != NULL (heads = 1)
 * W [out_cols, k] row-major (ldw); k <= 128 and k % 4 == 0; out_cols == 128.  Row strides in
 * floats, multiples of 4, 16-byte aligned rows.  fp32 MFMA (exact fp32 FMA chains). */
int ppgat_project_supported(int k, int out_cols);
int ppgat_project(const float* x0, int64_t ldx0, const float* x1, int64_t ldx1, int64_t split, int64_t n, int k,
                  const float* w, int64_t ldw, int out_cols, const float* bias, const float* att_src,
                  const float* att_dst, float* y, int64_t ldy, float* s_src, float* s_dst, void* stream);
/* Input gradient of the layer (heads = 1), from the message gradient D [n, k] (ldd) and the
 * node logit gradients S [n, 2] = {ds_src, ds_dst} (lds) of ppgat_bwd_edges +
 * ppgat_bwd_dst_sum:
 *   dx = D W + ds_src (x) (att_src W) + ds_dst (x) (att_dst W)
 * W [k, out_cols] row-major = lin.weight; k <= 128, out_cols == 128. */
int ppgat_project_bwd_input(const float* D, int64_t ldd, int64_t n, int k, const float* w, int64_t ldw, int out_cols,
                            const float* att_src, const float* att_dst, const float* S, int64_t lds, float* dx,
                            int64_t lddx, void* stream);
/* The heads = 1 layer's input gradient AND its weight-gradient products in one pass over D and
 * x (replaces, with the two calls above: the autograd of GATConv.lin / SimpleGATLayer.lin,
 * train_gat_pyg.py:77, train_gat_custom.py:77, for the x rows and the weight):
 *   dx = D W + ds_src (x) (att_src W) + ds_dst (x) (att_dst W)    (dx nullable: skipped)
 *   G  = D^T x [k, k],   GV = [ds_src^T x ; ds_dst^T x] [2, k]     (for ppgat_weight_grads)
 * x rows [0, split) from x0, [split, n) from x1 (x1 nullable).  Supported when k == 128 and
 * the split-bf16 GEMM family is on (ppgat_project_bwd_fused_supported); deterministic. */
int ppgat_project_bwd_fused_supported(int k);
int ppgat_project_bwd_fused_workspace_bytes(int64_t n, size_t* bytes);
int ppgat_project_bwd_fused(const float* D, int64_t ldd, const float* S, int64_t lds, const float* x0, int64_t ldx0,
                            const float* x1, int64_t ldx1, int64_t split, int64_t n, int k, const float* w,
                            int64_t ldw, const float* att_src, const float* att_dst, float* dx, int64_t lddx,
                            float* G, float* GV, void* workspace, size_t workspace_bytes, void* stream);
/* ppgat_project_bwd_fused (dx required) that also does the backward prologue of the layer that
 * produced x, when x IS that layer's output (heads = 1, no op in between: the stacked convs of
 * train_gat_pyg.py:86-87) and dx is its whole grad_out -- ppgat_bwd_prologue's outputs for that
 * layer, from dx while it is still on chip instead of a second pass over dx and x:
 *   prev_nstate[r] = {prev_s_dst[r], prev_m[r], prev_inv_l[r], prev_gscale <dx_r, x_r - prev_bias>}
 *   prev_grad_bias = sum_r dx_r                       (prev_bias / prev_grad_bias nullable)
 * Same dx, G, GV as ppgat_project_bwd_fused, bit for bit; deterministic. */
int ppgat_project_bwd_fused_producer(const float* D, int64_t ldd, const float* S, int64_t lds, const float* x0,
                                     int64_t ldx0, const float* x1, int64_t ldx1, int64_t split, int64_t n, int k,
                                     const float* w, int64_t ldw, const float* att_src, const float* att_dst,
                                     float* dx, int64_t lddx, float* G, float* GV, const float* prev_bias,
                                     const float* prev_s_dst, const float* prev_m, const float* prev_inv_l,
                                     float prev_gscale, float* prev_nstate, float* prev_grad_bias, void* workspace,
                                     size_t workspace_bytes, void* stream);
/* Weight and attention-vector gradients from G = dh_msg^T x [H*C, K] and
 * GV = [ds_src^T x ; ds_dst^T x] [2H, K] (ppgat_gemm_tn with V):
 *   dW = G + att_src (x) GV[:H] + att_dst (x) GV[H:],  datt_src[h] = W_h GV[h],  datt_dst[h] = W_h GV[H + h]. */
int ppgat_weight_grads(const float* G, const float* GV, const float* w, const float* att_src, const float* att_dst,
                       int heads, int channels, int in_channels, float* dW, float* datt_src, float* datt_dst,
                       void* stream);

/* ---- optimizer -------------------------------------------------------------------------
 * Replaces: torch.optim.Adam(model.parameters(), lr, weight_decay) .step()
 * (train_gat_pyg.py:299,323) for fp32 dense tensors, amsgrad=False, maximize=False:
 *   g += wd * p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2   ((1 - b) rounded from double);
 *   p -= step_size * m / (sqrt(v) / bias_correction2_sqrt + eps)
 * with step_size = lr / (1 - b1^t), bias_correction2_sqrt = sqrt(1 - b2^t) per tensor
 * (host arrays).  count <= ppgat_adam_max_tensors() tensors in one launch. */
int ppgat_adam_max_tensors(void);
int ppgat_adam_step(int count, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const int64_t* numel, const float* step_size,
                    const float* bias_correction2_sqrt, double beta1, double beta2, float eps, float weight_decay,
                    void* stream);
/* Graph-capturable variant: tensor k's step count t is read on the device from *step[k] (one
 * float per parameter, as torch.optim.Adam(capturable=True) keeps it; the caller increments
 * them on the same stream before the launch), step_size = lr / (1 - beta1^t)
 * and bias_correction2_sqrt = sqrt(1 - beta2^t) are formed in double in the kernel and
 * rounded once -- the values the host path passes.  Same replacement as ppgat_adam_step
 * (torch.optim.Adam(capturable=True) semantics); one launch per <= max_tensors tensors. */
int ppgat_adam_step_device(int count, float* const* params, const float* const* grads, float* const* exp_avg,
                           float* const* exp_avg_sq, const int64_t* numel, const float* const* step, double lr,
                           double beta1,
                           double beta2, float eps, float weight_decay, void* stream);
/* Row-sparse ("lazy") Adam -- torch.optim.SparseAdam's place, with Adam's own rule: for each k in
 * [0, n_rows), r = rows[k], ppgat_adam_step's element rule above on (param[r, c], grad_rows[k, c],
 * exp_avg[r, c], exp_avg_sq[r, c]) for every column c, with one step_size and
 * bias_correction2_sqrt for the table (its global step count).  param, exp_avg, exp_avg_sq:
 * [n_table_rows, dim] contiguous; grad_rows [n_rows, dim]; rows [n_rows] int64.  Rows not named in
 * rows are neither read nor written, so the update is lazy: untouched rows receive no momentum
 * step, and weight decay acts on touched rows only.
 * Contract: rows strictly ascending (hence unique: no two waves write one row) and inside
 * [0, n_table_rows).  The kernel checks both as it goes and ORs into *flag (sticky; flag may be
 * NULL): bit 1 = a row outside the range, which is skipped and never dereferenced; bit 2 =
 * rows[k] <= rows[k - 1].  A raised flag means the step's result is invalid, never an
 * out-of-bounds access.  The debug build validates the range of rows before the launch.
 * Refused before any launch: a NULL param / exp_avg / exp_avg_sq / grad_rows / rows, dim < 1, a
 * negative size -> PPGAT_ERR_INVALID; n_rows or n_table_rows >= 2^31 -> PPGAT_ERR_UNSUPPORTED.
 * n_rows == 0: PPGAT_OK, nothing launched.  Traffic: 8 + 28 dim bytes per touched row.
 * float4 accesses when dim % 4 == 0 and the four bases are 16-byte aligned.  Deterministic. */
int ppgat_adam_rows(float* param, float* exp_avg, float* exp_avg_sq, const float* grad_rows, const int64_t* rows,
                    int64_t n_rows, int64_t n_table_rows, int dim, float step_size, float bias_correction2_sqrt,
                    double beta1, double beta2, float eps, float weight_decay, int* flag, void* stream);

/* ---- replicated-item partition: cross-rank merge of item destination rows -----------------
 * Replaces: nothing one-to-one -- in the reference every destination's softmax sees all of
 * its in-edges (PyG softmax over edge_index, train_gat_pyg.py:77); with users sharded over
 * ranks and the item rows replicated (dist.py), an item's in-edges are split over the ranks,
 * so each rank's ppgat_fwd output for item rows is merged exactly (PyG mode, eps 1e-16):
 *   phase 0: mx[i,h] = m[i,h] if row i has local in-edges else -inf      -> all_reduce(MAX, mx)
 *   phase 1: pack = [c * a | c], c = (1/inv_l - eps) * exp(m - mx) (0 for rows without local
 *            in-edges), a = agg (heads > 1) or out - bias (heads = 1)     -> all_reduce(SUM, pack)
 *   phase 2: agg = pack_a / (pack_c + eps), out = mean_h agg + bias, inv_l = 1/(pack_c + eps),
 *            m = pack_c > 0 ? mx : 0   (in place on the item rows)
 * item_rowptr: the local CSR rowptr at the first item row (n_items + 1 entries); out/agg/m/inv_l
 * point at the first item row; pack holds n_items*heads*(channels + 1) floats ([a] then [c]). */
int ppgat_rep_merge(int phase, const int32_t* item_rowptr, int64_t n_items, int heads, int channels, float* out,
                    float* agg, const float* bias, float* m, float* inv_l, float* mx, float* pack, void* stream);

/* ---- row-sharded partition: halo exchange rows ------------------------------------------
 * Replaces: nothing one-to-one -- the reference is one process on one GPU; with nodes
 * row-sharded over ranks (dist.py ExchangePlan) every layer all_to_all's the rows the peers'
 * edges read, and the backward returns their gradients to the owner.
 *   ppgat_rows_gather:     dst[r, :] = src[idx[r], :]      (pack the all_to_all send buffer)
 *   ppgat_rows_return_add: dst[o, :] += sum_{k = ret_ptr[o]}^{ret_ptr[o+1]-1} ret[ret_pos[k], :]
 *                          (returned halo gradients, added in peer order: deterministic)
 * Rows of `cols` floats with row strides ld_* (floats). */
int ppgat_rows_gather(const float* src, int64_t ld_src, const int64_t* idx, int64_t n_rows, int cols, float* dst,
                      int64_t ld_dst, void* stream);
int ppgat_rows_return_add(float* dst, int64_t ld_dst, const float* ret, int64_t ld_ret, const int32_t* ret_ptr,
                          const int32_t* ret_pos, int64_t n_rows, int cols, void* stream);

/* ---- dropout epoch (hipGraph replays) ------------------------------------------------------
 * Every dropout mask of ppgat_fwd / ppgat_bwd_edges uses seed' = seed + epoch * 0xD1B54A32D192ED03
 * (mod 2^64), epoch a device-side counter (0 at load: seeds are used as passed).  A training
 * step captured once in a hipGraph bakes its host seeds in; enqueueing ppgat_dropout_advance
 * at the top of the captured step gives every replay fresh masks (the reference draws new
 * F.dropout masks per call, train_gat_pyg.py:77 attn dropout).  Stream-ordered.
 * Replaces: nothing in the reference (eager PyTorch draws from its generator each call). */
int ppgat_dropout_advance(void* stream);
int ppgat_dropout_set_epoch(uint64_t epoch, void* stream);

/* ---- I-I kNN graph (config 3's second relation) ------------------------------------
 * Replaces: the per-item selection loop of graphs/build_ii_knn.py:76-99 (self excluded as
 * -inf, argpartition top-k, sorted descending, kept where sim >= min_similarity).  S is a
 * block of the cosine-similarity matrix: rows = query items q0 .. q0 + rows - 1, columns =
 * all n_cols items (row stride ld floats).  Writes, per row, the k best (item, similarity)
 * sorted by similarity descending with ties by smaller item index (out_idx / out_sim
 * [rows, k]; -1 / -inf where fewer than k items exist) and out_cnt[row] = how many of them
 * reach min_sim, sim >= min_sim (a prefix).  An entry of S that is -inf or NaN is absent, like
 * the item itself (column q0 + row; q0 = n_cols means no column is the item): it is never
 * selected, whatever k, and never counted.  The -1 / -inf pads are not items and are not
 * counted either, so with min_sim = -inf out_cnt is the number of items written.  Columns n_cols .. ld - 1 are never read.
 * Refused with nothing written: k outside [1, ppgat_knn_max_k()] (PPGAT_ERR_UNSUPPORTED),
 * n_cols < 1, ld < n_cols, q0 < 0 (PPGAT_ERR_INVALID).  Deterministic. */
int ppgat_knn_max_k(void);
int ppgat_knn_topk(const float* S, int64_t ld, int64_t rows, int64_t n_cols, int64_t q0, int k, float min_sim,
                   int32_t* out_idx, float* out_sim, int32_t* out_cnt, void* stream);

/* ---- BPR triple sampler ---------------------------------------------------------------
 * Replaces: sample_bpr_epoch, scripts/train_gat_pyg.py:179-190 (Python loop per epoch):
 *   u uniform over users with >= 1 train item; i uniform over the positions of u's train
 *   list (random.choice); j uniform over [0, n_items), redrawn while j is one of u's items.
 * Same distribution, a counter-based stream instead of Python's Mersenne twister: every
 * draw hashes (seed, t0 + s, draw number), so a triple does not depend on how the S
 * triples are split over calls (oracle/sampler_oracle.py restates the stream bit for bit).
 * prepare (once per graph): user_ptr [n_users+1] int64 CSR over user_items [nnz] int32 item
 * ids (any order within a user) -> items_sorted [nnz] (each user's items ascending),
 * eligible [n_users] (ids of users with items, ascending) and *n_eligible (device int64).
 * sample: u, i, j [S] int64; *bad (device) = 1 if no user has items, 2 if some user's
 * negative was not found in 1024 draws (the user holds ~all items; the reference loops). */
int ppgat_bpr_sampler_workspace_bytes(int64_t n_users, int64_t nnz, size_t* bytes);
int ppgat_bpr_sampler_prepare(const int64_t* user_ptr, const int32_t* user_items, int64_t n_users, int64_t nnz,
                              int32_t* items_sorted, int32_t* eligible, int64_t* n_eligible, void* workspace,
                              size_t workspace_bytes, void* stream);
int ppgat_bpr_sample(const int64_t* user_ptr, const int32_t* items_sorted, const int32_t* eligible,
                     const int64_t* n_eligible, int64_t n_items, int64_t n_triples, uint64_t seed, int64_t t0,
                     int64_t* u, int64_t* i, int64_t* j, int32_t* bad, void* stream);

/* ---- BPR mini-batches: every positive x neg_per_pos ------------------------------------
 * Replaces: sample_bpr_batches, scripts/train_lightgcn.py:160-179 (a Python loop over every
 *   train interaction per epoch): users in order, each user's items in list order,
 *   neg_per_pos negatives each, cut into batches of batch_size triples.
 * Triple t in [t0, t0 + n_triples), t0 + n_triples <= nnz * neg_per_pos: p = t / neg_per_pos,
 * u = the user whose range of user_ptr holds p, i = user_items[p] (the ORIGINAL order given
 * to ppgat_bpr_sampler_prepare, which is the reference's enumeration order), j = the first
 * draw d = 0, 1, ... of the counter stream (seed, t, d) that is not one of u's items
 * (items_sorted of ppgat_bpr_sampler_prepare; same hash, range reduction, 1024-draw limit and
 * *bad = 2 rule as ppgat_bpr_sample).  Batch b of an epoch: t0 = b * batch_size, n_triples =
 * min(batch_size, nnz * neg_per_pos - t0); the (u, i) columns then equal the reference's
 * batches exactly, j comes from the counter stream instead of Python's random. */
int ppgat_bpr_sample_positives(const int64_t* user_ptr, const int32_t* user_items, const int32_t* items_sorted,
                               int64_t n_users, int64_t nnz, int64_t n_items, int64_t neg_per_pos, int64_t n_triples,
                               uint64_t seed, int64_t t0, int64_t* u, int64_t* i, int64_t* j, int32_t* bad,
                               void* stream);

/* ---- LightGCN propagation hop -------------------------------------------------------------
 * Replaces: one iteration of LightGCN.propagate, scripts/train_lightgcn.py:69-72
 *   (A = torch.sparse_coo_tensor(...); out = torch.sparse.mm(A, out); acc = acc + out) and, on
 *   the last hop, the layer mean acc / (K + 1) of :73; with the CSC view, their autograd.
 * For every row i of a CSR (sched over its rowptr, col [n_edges], val [n_edges] per slot):
 *   s_i     = sum over the slots k of row i, in slot order, of val[k] * src[col[k]]  (fp32 FMAs)
 *   out[i]  = s_i                          when out  != NULL
 *   accw[i] = (acc_in[i] + s_i) / div      when accw != NULL  (acc0 == NULL: acc_in = 0;
 *                                          IEEE division, skipped when div == 1)
 * src [n_src, channels] and acc_in [n_rows, channels] may each be two row segments: rows
 * [0, split) at the first pointer, the rest at the second (second NULL: one segment), so hop 1
 * reads E_user.weight and E_item.weight where they are.  accw may be acc_in's buffer (in
 * place); out and accw must not be the gathered table.  channels in {64, 128, 256}
 * (ppgat_lgcn_supported).  workspace: the hub pieces' partial rows, added in piece order.
 * Atomic-free: two launches give the same bits.  A K-hop propagate is K calls: hop 1 with
 * acc_in = x0 writing out_1 and acc, middle hops updating acc in place, hop K writing only the
 * result with div = K + 1.  The gradient with respect to x0 is the same K calls over the CSC
 * view (bwd schedule, row, val_t = val[csc2csr]) applied to the incoming gradient. */
int ppgat_lgcn_supported(int channels);
int ppgat_lgcn_hop_workspace_bytes(int64_t n_hub_items, int channels, size_t* bytes);
int ppgat_lgcn_hop(const ppgat_schedule* sched, const int32_t* col, const float* val, int64_t n_rows, int64_t n_src,
                   int64_t n_edges, int channels, const float* src0, const float* src1, int64_t src_split,
                   const float* acc0, const float* acc1, int64_t acc_split, float div, float* out, float* accw,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- GATv2 dynamic-attention layer ----------------------------------------------------------
 * Replaces: torch_geometric.nn.GATv2Conv (Brody et al., "How Attentive are Graph Attention
 *   Networks?") with concat=False, add_self_loops=False, edge_dim=None, residual=False, after
 *   its projections x_l = lin_l(x), x_r = lin_r(x) (both [N, H, C]; x_r may be x_l's buffer,
 *   share_weights).  Per edge j -> i and head h:
 *     t_ij  = x_l[j] + x_r[i];   e_ij = sum_c att[h,c] * leaky_relu(t_ij[c], negative_slope)
 *     alpha = exp(e_ij - max_i) / (sum over the in-edges of i of exp(e - max_i) + 1e-16)
 *     out_i = mean_h sum_j mask_ij alpha_ij x_l[j] + bias     (no in-edges: exactly bias)
 *   mask is ppgat_fwd's counter-hash dropout multiplier of (effective seed, original edge
 *   column, head, dropout_p).  The C entries carry "dynatt" in their names (the symbol check of
 *   this header admits lower-case letters and underscores only).
 * ppgat_dynatt_supported: 1 for (heads, channels) in {(1,32), (1,64), (1,128), (2,64), (2,128),
 *   (4,64), (4,128)}; every other shape returns PPGAT_ERR_UNSUPPORTED before any device work.
 * ppgat_dynatt_workspace_bytes: backward == 0: the forward's hub-piece states (n_dst_hub_items
 *   of the CSR schedule); backward != 0: node state, dbias / datt partial rows and the hub
 *   pieces' partial sums and rows of the passes.  Host only.
 * ppgat_dynatt_fwd: dst_sched over the CSR by destination.  Writes out [N,C], m and inv_l =
 *   1/(l + 1e-16) [N,H] (saved for the backward).  seed_used (device uint64[1]) is required
 *   when dropout_p > 0 and receives the effective seed (seed folded with the dropout epoch),
 *   which the kernels read from there.
 * ppgat_dynatt_bwd: src_sched over the CSC by source, dst_sched over the CSR by destination.
 *   Given grad_out [N,C] returns grad_x_l and grad_x_r [N,H,C] (two buffers even when x_r is
 *   x_l: the caller adds them), grad_att [H,C] and, when grad_bias != NULL, grad_bias [C].  A
 *   sweep by destination sums D_i = sum_j alpha_ij dalpha_ij edge by edge (not g_i . agg_i: the
 *   softmax backward's cancellation is then exact for a single in-edge), one pass by source
 *   owns grad_x_l[j], one by destination owns grad_x_r[i] and recomputes the logit gradient from
 *   grad_out[i] . x_l[j]; grad_att and grad_bias are per-block partial rows summed in block
 *   order.  No float atomics: two calls give the same bits.  seed_used: the forward's (required
 *   when dropout_p > 0), so the backward regenerates the forward's mask.  No entry synchronises
 *   the host. */
int ppgat_dynatt_supported(int heads, int channels);
int ppgat_dynatt_workspace_bytes(int64_t n_nodes, int64_t n_dst_hub_items, int64_t n_src_hub_items, int heads,
                                 int channels, int backward, size_t* bytes);
int ppgat_dynatt_fwd(const ppgat_schedule* dst_sched, const int32_t* col, const int32_t* csr_eid, int64_t n_nodes,
                     int64_t n_edges, int heads, int channels, const float* x_l, const float* x_r, const float* att,
                     const float* bias, float negative_slope, float dropout_p, uint64_t seed, uint64_t* seed_used,
                     float* out, float* m, float* inv_l, void* workspace, size_t workspace_bytes, void* stream);
int ppgat_dynatt_bwd(const ppgat_schedule* src_sched, const ppgat_schedule* dst_sched, const int32_t* row,
                     const int32_t* csc_eid, const int32_t* col, const int32_t* csr_eid, int64_t n_nodes,
                     int64_t n_edges, int heads, int channels, const float* x_l, const float* x_r, const float* att,
                     const float* m, const float* inv_l, const float* grad_out, float negative_slope,
                     float dropout_p, const uint64_t* seed_used, float* grad_x_l, float* grad_x_r, float* grad_att,
                     float* grad_bias, void* workspace, size_t workspace_bytes, void* stream);

/* ---- attention weights and the most-attended neighbours ---------------------------------
 * Replaces: the alpha of torch_geometric's return_attention_weights=True (GATConv, GATv2Conv),
 *   and a per-destination sort of it.  alpha [E, H] is the forward's softmax weight BEFORE the
 *   dropout mask, recomputed per edge from the forward's own final state m and inv_l [N, H]:
 *     PyG mode     alpha = exp(e - m_i) * inv_l_i,  e = leaky_relu((s_src[j] + s_dst[i]) [+ edge_term[k]])
 *     custom mode  alpha = exp(clamp(leaky_relu(z), -10, 10)) * inv_l_i     (no max subtraction)
 *     GATv2        e = att_h . leaky_relu(x_l[j] + x_r[i]),  alpha = exp(e - m_i) * inv_l_i
 *   with the arithmetic of the forward kernels, so that given the s_src / s_dst (x_l / x_r) the
 *   state was computed from, e - m <= 0 for every edge and a destination's largest weight is
 *   inv_l_i bit for bit.  There is no second reduction: hub pieces need no merge, no workspace.
 * order = 0: alpha[slot] (CSR slot order); order = 1: alpha[csr_eid[slot]] (the caller's
 *   edge_index column order; csr_eid required).  Every element of alpha is written exactly once.
 * ppgat_attention: dst_sched, col, csr_eid of the CSR by destination; s_src [>= max col + 1, H];
 *   s_dst, m, inv_l [n_nodes, H]; edge_term [E, H] in CSR slot order or NULL; heads <= 8 in
 *   either mode (the forward's custom mode is heads == 1; this entry reads whatever state it is
 *   given).
 * ppgat_dynatt_attention: the (heads, channels) of ppgat_dynatt_supported, others
 *   PPGAT_ERR_UNSUPPORTED before any device work; x_l, x_r [n_nodes, H, C], att [H, C].
 * ppgat_attention_topk: per destination i (one wave each, walking the whole row), the k (1..32)
 *   in-edges with the largest v = (sum_h val[slot, h]) * (1 / heads), val [E, H] in CSR slot
 *   order, ranked exactly under (v descending, original edge id ascending; NaN ranks as -inf):
 *   out_eid [N, k] the original edge ids (csr_eid; -1 pads), out_val [N, k] their v (0 in the
 *   pads), out_cnt [N] = min(k, in-degree).  It ranks whatever [E, H] array it is given.
 * All three validate on the host first (PPGAT_ERR_INVALID / PPGAT_ERR_UNSUPPORTED with nothing
 * launched), use no float atomics (two calls give the same bits) and never synchronise. */
int ppgat_attention(const ppgat_schedule* dst_sched, const int32_t* col, const int32_t* csr_eid,
                    const float* edge_term, int64_t n_nodes, int64_t n_edges, int heads, const float* s_src,
                    const float* s_dst, const float* m, const float* inv_l, int mode, float negative_slope,
                    int order, float* alpha, void* stream);
int ppgat_dynatt_attention(const ppgat_schedule* dst_sched, const int32_t* col, const int32_t* csr_eid,
                           int64_t n_nodes, int64_t n_edges, int heads, int channels, const float* x_l,
                           const float* x_r, const float* att, const float* m, const float* inv_l,
                           float negative_slope, int order, float* alpha, void* stream);
int ppgat_attention_topk(const int32_t* rowptr, const int32_t* csr_eid, const float* val, int64_t n_nodes,
                         int64_t n_edges, int heads, int k, int32_t* out_eid, float* out_val, int32_t* out_cnt,
                         void* stream);

/* ---- sampled-evaluation candidates ---------------------------------------------------
 * Replaces: the candidate draw of eval_sampled, scripts/train_gat_pyg.py:157-167 (a Python
 *   loop over ~192k users: np.random.randint(0, n_items) redrawn while the item is in the
 *   user's train set or is the held-out positive, eval_neg_k times per user).
 * cands [n_eval, n_neg + 1] int64: column 0 = pos[b], column 1 + k = the first draw d of the
 * counter-based stream (seed, t = b * n_neg + k, d) outside u's train items (items_sorted /
 * user_ptr of ppgat_bpr_sampler_prepare) and != pos[b] (oracle/sampler_oracle.py restates it);
 * *bad = 2 if some negative was not found in 1024 draws. */
int ppgat_eval_sample(const int64_t* user_ptr, const int32_t* items_sorted, const int64_t* users, const int64_t* pos,
                      int64_t n_eval, int64_t n_neg, int64_t n_items, uint64_t seed, int64_t* cands, int32_t* bad,
                      void* stream);

/* ---- weighted draws: negatives in proportion to item weights ----------------------------
 * Replaces: nothing in the reference, which draws every negative uniformly.
 * cdf uint64 [n_items] (device): the inclusive prefix sum of integer item weights w_i >= 0
 * quantised on the host, cdf[n_items - 1] = total > 0.  A draw is
 *   r = mulhi64(draw64(seed, t, d), total);  item = the first i with cdf[i] > r
 * (a binary search of the table), so item i comes with probability w_i / total exactly as far as
 * the 64-bit stream is uniform, and an item of weight 0 never comes.
 * ppgat_weighted_draws: out[n] = the draw (seed, t0 + n, 0), n < n_draws.
 * ppgat_weighted_bpr_sample: ppgat_bpr_sample's contract; u and i are bit for bit what it gives
 *   for the same (seed, t0 + s); j is the first weighted draw 2 + k outside u's items.
 * ppgat_weighted_eval_sample: ppgat_eval_sample's contract with weighted draws d = 0, 1, ...
 * 1024 draws at the most per negative, then 0 is written and *bad |= 2. */
int ppgat_weighted_draws(const uint64_t* cdf, int64_t n_items, int64_t n_draws, uint64_t seed, int64_t t0,
                         int64_t* out, void* stream);
int ppgat_weighted_bpr_sample(const int64_t* user_ptr, const int32_t* items_sorted, const int32_t* eligible,
                              const int64_t* n_eligible, int64_t n_items, const uint64_t* cdf, int64_t n_triples,
                              uint64_t seed, int64_t t0, int64_t* u, int64_t* i, int64_t* j, int32_t* bad,
                              void* stream);
int ppgat_weighted_eval_sample(const int64_t* user_ptr, const int32_t* items_sorted, const int64_t* users,
                               const int64_t* pos, int64_t n_eval, int64_t n_neg, int64_t n_items,
                               const uint64_t* cdf, uint64_t seed, int64_t* cands, int32_t* bad, void* stream);

/* ---- fan-out neighbour sampling: a per-epoch sampled graph, derived without a sort --------
 * Replaces: nothing in the reference, which trains on the whole graph at every step; the path it
 *   spares is ppgat_csr_build (two radix sorts) over a resampled edge_index each epoch.
 * The rule.  Destination i with in-degree d = rowptr[i + 1] - rowptr[i] and cap f (f = fanout,
 *   or fanout_of[i] where fanout_of is given and its entry is >= 0; an entry < 0 keeps all; 0
 *   keeps nothing) numbers its in-edges p = 0 .. d - 1 in CSR slot order (ascending original edge
 *   id: the build's sort is stable).  d <= f keeps every in-edge.  d > f keeps the positions of
 *   Robert Floyd's subset S over the counter stream of ppgat_bpr_sample:
 *     S = {};  for s = 0 .. f - 1:  j = d - f + s;  t = mulhi64(draw64(seed, i, s), j + 1);
 *                                   add (t in S ? j : t) to S
 *   so every f-subset is equally likely, a row's sample depends on (seed, i, d, f) alone -- never
 *   on the launch geometry -- and a row costs f draws, not d.  One wave per such row: lane s
 *   holds element s of S and membership is a compare plus a 64-bit ballot, hence
 *   f <= ppgat_neighbor_max_fanout() = 64.  Rows with d <= f are copied by a streaming pass over
 *   the sampled slots and pay no wave.
 * The sampled graph: its edges are the kept ones in ascending original edge id, renumbered
 *   0 .. E' - 1 (new id = exclusive scan of the keep flags in edge-id order).  Every array written
 *   equals, element for element, what ppgat_csr_build gives for edge_index_s, and
 *   csr2csc_s what ppgat_invert_index gives for csc2csr_s.
 * Three calls on one stream share one workspace (ppgat_neighbor_sample_workspace_bytes(n_nodes,
 * n_edges), host-only), which the caller leaves untouched between them:
 * ppgat_neighbor_count: rowptr_s [n_nodes + 1] = exclusive scan of min(d, f); info [2] int32 =
 *   {E' = rowptr_s[n_nodes], bad}; bad = 1 if some fanout_of entry exceeds the maximum (that row
 *   is then counted as if capped at the maximum and the caller must not go on).  The caller's
 *   read of info is the only host sync these entries need: E' sizes the outputs of the other two.
 * ppgat_neighbor_sample: rowptr, col, csr_eid [n_edges] the parent's CSR, csr2csc [n_edges] the CSC
 *   slot of each CSR slot (ppgat_invert_index of csc2csr), edge_index [2, n_edges] int64 what the
 *   parent was built from, rowptr_s and n_kept = E' from the count.  Writes col_s,
 *   csr_eid_s [E'] (new numbering), edge_index_s [2, E'] int64 (the kept columns) and eid [E']
 *   int64 (their original ids, so edge_attr[eid] is the sampled graph's attribute tensor).
 * ppgat_neighbor_derive: colptr, row, csc_eid, csc2csr the parent's CSC.  Writes colptr_s
 *   [n_nodes + 1], row_s, csc_eid_s, csc2csr_s, csr2csc_s [E'] (a scan of the keep flags the
 *   pick left in CSC order, plus a scatter).  The schedules are ppgat_schedule_build over rowptr_s / colptr_s.
 * Refused before any device work: fanout outside [1, max] -> PPGAT_ERR_UNSUPPORTED; a negative
 *   size, n_kept > n_edges, a NULL required pointer (the per-edge ones only when n_edges, resp.
 *   n_kept, > 0; fanout_of may be NULL) or a short workspace -> PPGAT_ERR_INVALID; sizes >= 2^31
 *   -> PPGAT_ERR_UNSUPPORTED.  No float anywhere, no atomics on data: two calls give the same
 *   bits.  Nothing past an output's stated length is written.  The debug build validates
 *   rowptr / colptr / rowptr_s and the parent's index arrays first. */
int ppgat_neighbor_max_fanout(void);
int ppgat_neighbor_sample_workspace_bytes(int64_t n_nodes, int64_t n_edges, size_t* bytes);
int ppgat_neighbor_count(const int32_t* rowptr, int64_t n_nodes, int64_t n_edges, int fanout,
                         const int32_t* fanout_of, int32_t* rowptr_s, int32_t* info, void* workspace,
                         size_t workspace_bytes, void* stream);
int ppgat_neighbor_sample(const int32_t* rowptr, const int32_t* col, const int32_t* csr_eid,
                          const int32_t* csr2csc, const int64_t* edge_index, int64_t n_nodes, int64_t n_edges, uint64_t seed,
                          const int32_t* rowptr_s, int64_t n_kept, int32_t* col_s, int32_t* csr_eid_s,
                          int64_t* edge_index_s, int64_t* eid, void* workspace, size_t workspace_bytes,
                          void* stream);
int ppgat_neighbor_derive(const int32_t* colptr, const int32_t* row, const int32_t* csc_eid, const int32_t* csc2csr,
                          int64_t n_nodes, int64_t n_edges, int64_t n_kept, int32_t* colptr_s, int32_t* row_s,
                          int32_t* csc_eid_s, int32_t* csc2csr_s, int32_t* csr2csc_s, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- seed-subgraph sampling: the L-hop sampled in-neighbourhood of a seed set ---------------
 * Replaces: nothing in the reference, which trains on the whole graph at every step.  What PyG
 *   calls NeighborLoader: a mini-batch names its seed nodes, only their sampled neighbourhood is
 *   extracted and relabelled into a small graph, and the step's work scales with the batch.
 * The rule.  Inputs: the parent graph over n_nodes nodes, the cap rule above (fanout, fanout_of), a
 *   64-bit seed, seed nodes T (int64, any order, duplicates allowed), hops = L in [0, 8].  Let S be
 *   the edge set the fan-out sampler keeps under (fanout, fanout_of, seed): a row's sample depends
 *   on (seed, i, d, f) alone, i the node's GLOBAL id, so the subgraph is a restriction of S.
 *     depth(v) = 0 for v in T; else 1 + the least depth of a destination v feeds through an edge
 *                of S; unreached nodes have none.
 *     V = {depth <= L};  X = {depth < L}, the expanded nodes.
 *     K = {e in S : dst(e) in X}, so every source of K is in V.
 *     n_id = V ascending (users precede items); a node's local id is its position in n_id; the
 *     kept edges stay in ascending original edge id.
 *   L = 0 gives the unique seeds and no edges; an empty T gives an empty subgraph.
 * Outputs: n_id [N_s] int64, depth [N_s] int32, n_users_s = #{n_id < n_users}, edge_index_s
 *   [2, E_s] int64 in local ids, eid [E_s] int64 (the original columns), seed_local [n_seeds] int64
 *   in the order of T, and the CSR / CSC views over N_s nodes, every array equal, element for
 *   element, to ppgat_csr_build of edge_index_s.  Relabelling is monotone, so the views are
 *   compactions of the parent's (no sort): the edge side is ppgat_neighbor_count / _sample /
 *   _derive under a cap table that is 0 outside X, the node side a scan of the reached flags.
 * The calls, on one stream, share one workspace (ppgat_subgraph_workspace_bytes(n_nodes),
 * host-only) which the caller leaves untouched between them:
 * ppgat_subgraph_seed: clears info [4] int32 and the depths, gives every seed depth 0; a seed
 *   outside [0, n_nodes) sets info[2] = 1 (and is otherwise ignored).
 * ppgat_subgraph_expand, once per hop = 0 .. L - 1 in order: the rows of depth hop give depth
 *   hop + 1 to the sources of their kept slots that have none (rowptr, col: the parent's CSR).
 * ppgat_subgraph_plan: cap [n_nodes] int32 = the cap of the rows in X (fanout, or the row's
 *   fanout_of entry as it stands), 0 elsewhere -- the fanout_of of the ppgat_neighbor_count call
 *   that follows; info[0] = N_s, info[1] = n_users_s; info[3] = 1 if any fanout_of entry exceeds
 *   the maximum.  The caller reads info together with ppgat_neighbor_count's: the one host sync.
 * ppgat_subgraph_relabel, after ppgat_neighbor_sample / _derive wrote rowptr_p, colptr_p
 *   [n_nodes + 1], col_s, row_s [n_kept] and edge_index_s [2, n_kept] in parent ids: writes n_id,
 *   depth [n_sub], rowptr_s, colptr_s [n_sub + 1], seed_local [n_seeds], and relabels col_s, row_s
 *   and edge_index_s in place.  n_sub = N_s and n_kept = E_s as read from the info arrays.
 * Refused before any device work: fanout outside [1, max] -> PPGAT_ERR_UNSUPPORTED; hop outside
 *   [0, 8), hops outside [0, 8], a negative size, n_users or n_sub above n_nodes, a NULL required
 *   pointer (the per-node, per-edge and per-seed ones only when that count is > 0; fanout_of may
 *   be NULL) or a short workspace -> PPGAT_ERR_INVALID; sizes >= 2^31 -> PPGAT_ERR_UNSUPPORTED.
 *   Integers only, no atomics: a depth or a flag may be stored by several threads, always with
 *   the same value, so two calls give the same bits.  Nothing past an output's stated length is
 *   written. */
int ppgat_subgraph_max_hops(void);
int ppgat_subgraph_workspace_bytes(int64_t n_nodes, size_t* bytes);
int ppgat_subgraph_seed(const int64_t* seeds, int64_t n_seeds, int64_t n_nodes, int32_t* info, void* workspace,
                        size_t workspace_bytes, void* stream);
int ppgat_subgraph_expand(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int64_t n_edges, int hop,
                          int fanout, const int32_t* fanout_of, uint64_t seed, void* workspace,
                          size_t workspace_bytes, void* stream);
int ppgat_subgraph_plan(int64_t n_nodes, int64_t n_users, int hops, int fanout, const int32_t* fanout_of,
                        int32_t* cap, int32_t* info, void* workspace, size_t workspace_bytes, void* stream);
int ppgat_subgraph_relabel(int64_t n_nodes, int64_t n_sub, int64_t n_kept, const int64_t* seeds, int64_t n_seeds,
                           const int32_t* rowptr_p, const int32_t* colptr_p, int64_t* n_id, int32_t* depth,
                           int32_t* rowptr_s, int32_t* colptr_s, int32_t* col_s, int32_t* row_s,
                           int64_t* edge_index_s, int64_t* seed_local, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- sampled ranking (evaluation) ------------------------------------------------
 * Replaces: the per-user loop of eval_sampled, scripts/train_gat_pyg.py:160-175:
 *   scores = I[cands[b]] @ U[users[b]];  rank[b] = #(scores[1:] > scores[0]) + 1
 * cands [n_eval, n_cand] int64 item ids (column 0 = the held-out positive); Z rows as in
 * ppgat_bpr_fwd (row_map nullable).
 */
int ppgat_sampled_rank(const float* Z, int64_t n_rows, int64_t n_users, int64_t n_items, const int32_t* row_map,
                       int channels, const int64_t* users, const int64_t* cands, int64_t n_eval, int64_t n_cand,
                       int32_t* rank, void* stream);

/* ---- full-catalogue ranking (evaluation) ---------------------------------------------
 * The full-ranking protocol of the LightGCN literature: the held-out positive against EVERY
 * item outside the user's train history, not against sampled negatives.  For entry b, with
 * u = users[b], p = pos[b], X = history(u) + {p} and s(i) = <user_rows[u], item_rows[i]>:
 *   rank[b] = 1 + #{ i not in X : s(i) > s(p) }      (strict, scripts/train_gat_pyg.py:171)
 *   ties[b] =     #{ i not in X : s(i) == s(p) }     (nullable; a collapsed model shows here)
 * Exclusion is by index: the positive's own column is never compared, a history item is dropped
 * whatever its score, duplicates in a history or a history that holds p change nothing.  Users
 * may repeat; an empty history is legal.  user_ptr [n_users + 1] / items_sorted: the train
 * history CSR with each user's items ascending (ppgat_bpr_sampler_prepare's outputs); both NULL
 * = no history.  Rows: ld_user, ld_item >= channels, 16-byte aligned; the two tables may be
 * row ranges of one node table.  channels in {32, 64, 128, 256} (ppgat_full_rank_supported).
 * One fused pass on the matrix cores (bf16 three-term split, fp32 accumulation: fp32 dot-product
 * accuracy); the score matrix is never written.  Integer adds only: exact and repeatable.
 * s(p) goes through the same product as every s(i), so equal rows give bitwise equal scores.
 * The workspace is unused (0 bytes are reported); n_eval == 0 succeeds without a launch. */
int ppgat_full_rank_supported(int channels);
int ppgat_full_rank_workspace_bytes(int64_t n_eval, int64_t n_items, int channels, size_t* bytes);
int ppgat_full_rank(const float* user_rows, int64_t ld_user, int64_t n_users, const float* item_rows, int64_t ld_item,
                    int64_t n_items, int channels, const int64_t* users, const int64_t* pos, int64_t n_eval,
                    const int64_t* user_ptr, const int32_t* items_sorted, int32_t* rank, int32_t* ties,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- full-catalogue top-K (recommendation) -------------------------------------------
 * The recommender's output: for query b, with u = users[b] (users == NULL: query b is user b,
 * n_query <= n_users) and s(i) = <user_rows[u], item_rows[i]>, the k best items outside
 * history(u) under the total order (score descending, item index ascending):
 *   out_idx [n_query, k] int32, out_score [n_query, k] fp32 (nullable), best first;
 *   fewer than k eligible items: the tail is -1 / -inf.
 * Exclusion is by index, with ppgat_full_rank's CSR (user_ptr / items_sorted of
 * ppgat_bpr_sampler_prepare; both NULL = no history); duplicates in a history change nothing,
 * an empty history is legal, users may repeat.  Rows and channels as in ppgat_full_rank; NaN
 * scores are outside the contract.  1 <= k <= ppgat_full_topk_max_k() (128).
 * ppgat_full_rank's product with a selection epilogue: the score matrix is never written, and a
 * (user, item) score is bitwise the one ppgat_full_rank compares.  No float atomics: the lists are
 * a function of the total order alone, so two calls give the same bits.  The workspace
 * (ppgat_full_topk_workspace_bytes, sized for the current device: its CU count decides how the
 * item range is split) holds the candidate buffers, 8-byte aligned.  n_query == 0 succeeds
 * without a launch. */
int ppgat_full_topk_max_k(void);
int ppgat_full_topk_supported(int channels);
int ppgat_full_topk_workspace_bytes(int64_t n_query, int64_t n_items, int channels, int k, size_t* bytes);
int ppgat_full_topk(const float* user_rows, int64_t ld_user, int64_t n_users, const float* item_rows, int64_t ld_item,
                    int64_t n_items, int channels, const int64_t* users, int64_t n_query, const int64_t* user_ptr,
                    const int32_t* items_sorted, int k, int32_t* out_idx, float* out_score, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- serving top-K ------------------------------------------------------------------
 * Replaces: RecommenderRuntime.top_k_for_user_items, serving/runtime.py:56-76 (numpy):
 *   user_vec = mean(item_vecs[history]); scores = item_vecs @ user_vec; scores[history] = -1e9;
 *   the k best, descending.
 * Batched over n_users (<= 256) histories given as CSR (hist_ptr [n_users + 1] int64 into
 * hist_items; max_hist = the longest history).  The mean adds the history rows in order and
 * divides by the count (numpy's float32 mean over axis 0); ties between equal scores go to
 * the smaller item index (a total order).  out_idx/out_score [n_users, k]. */
int ppgat_serve_topk_workspace_bytes(int64_t n_items, int channels, int n_users, size_t* bytes);
int ppgat_serve_topk(const float* item_vecs, int64_t n_items, int channels, const int64_t* hist_ptr,
                     const int64_t* hist_items, int64_t max_hist, int n_users, int k, int32_t* out_idx,
                     float* out_score, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fusion MLP inference on the matrix cores (north star's MFMA target) ----------
 * Replaces: FusionMLP.forward + the normalisation and the per-row image copy loop of the
 *           inference pass, embeddings/fuse_modal.py:18-36,227-241:
 *   out = normalize?(relu([txt | img_row] W1^T + b1) W2^T + b2)   (norm: y / (||y|| + 1e-8))
 * img_row = img[img_index[b]] when img_index != NULL and img_index[b] >= 0, img_fallback
 * (the mean image embedding) when img_index[b] < 0, img[b] when img_index == NULL.
 * z1 (nullable) receives the pre-activation [n, hidden] for a training backward.
 * fp32 MFMA (exact fp32 FMA chains).  hidden_dim must be 256, output_dim 128, text_dim and
 * img_dim multiples of 32 (the reference's 384 + 512 -> 256 -> 128).
 */
int ppgat_fusion_fwd(const float* txt, const float* img, const int32_t* img_index, const float* img_fallback,
                     int64_t n, int text_dim, int img_dim, const float* w1, const float* b1, int hidden_dim,
                     const float* w2, const float* b2, int output_dim, int normalize, float* out, float* z1,
                     void* stream);
/* The same with a caller workspace (ppgat_fusion_fwd_workspace_bytes, 16-byte aligned): W1 and
 * W2 are split into their bf16 images once per call and the kernel stages them straight into
 * LDS (8 waves per workgroup share each staged chunk); bitwise the results of
 * ppgat_fusion_fwd. */
int ppgat_fusion_fwd_workspace_bytes(int text_dim, int img_dim, int hidden_dim, int output_dim, size_t* bytes);
int ppgat_fusion_fwd_ws(const float* txt, const float* img, const int32_t* img_index, const float* img_fallback,
                        int64_t n, int text_dim, int img_dim, const float* w1, const float* b1, int hidden_dim,
                        const float* w2, const float* b2, int output_dim, int normalize, float* out, float* z1,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- fusion MLP training: InfoNCE loss and backward, ReLU + dropout -----------------------
 * Replaces: contrastive_fusion_loss + its autograd backward, embeddings/fuse_modal.py:39-72
 *           (called by the training loop :179-214), and the ReLU/Dropout(0.1) of FusionMLP.mlp
 *           (:27-29) in train mode.  The Linear layers around them run on ppgat_gemm_nn /
 *           ppgat_gemm_tn_big / ppgat_colsum.
 * ppgat_infonce: F = fused, T = txt_proj(txt), I = img_proj(img), each [B, D] (D = 128,
 *   B <= 4096).  Fn, Tn, In = rows / max(||row||, 1e-12) (F.normalize); S_t = Fn Tn^T / tau,
 *   S_i = Fn In^T / tau; loss_t = mean_b CE(S_t[b], b), loss_i likewise.
 *   loss[3] = {(loss_t + loss_i) / 2, loss_t, loss_i} (device); dF, dT, dI = d loss / d(F, T, I).
 *   Fixed-order reductions (deterministic).  Workspace queried first.
 * ppgat_relu_dropout: backward 0: a = relu(z) * mask; backward 1: a <- a * mask * [z > 0] in place
 *   (a holds dL/da on entry).  mask = 0 with probability p, else 1 / (1 - p), from a counter hash
 *   of (seed, element index) -- the same draw forward and backward; p = 0 is plain ReLU. */
int ppgat_infonce_workspace_bytes(int64_t batch, int dim, size_t* bytes);
int ppgat_infonce(const float* fused, const float* txt_p, const float* img_p, int64_t batch, int dim, float tau,
                  float* loss, float* d_fused, float* d_txt_p, float* d_img_p, void* workspace, size_t workspace_bytes,
                  void* stream);
int ppgat_relu_dropout(const float* z, int64_t n, float p, uint64_t seed, int backward, float* a, void* stream);

/* ---- fp32 matrix-core GEMMs (v_mfma_f32_32x32x2_f32, exact fp32 FMA chains) ---------------
 * Replaces: the hipBLAS/cuBLAS GEMMs of torch.nn.Linear in GATConv.lin at shapes past the fused
 *           128-column projection (config 5: lin 256 -> 1024, train_gat_pyg.py:77) and of
 *           PyGGAT.item_proj (train_gat_pyg.py:74,81), and their weight gradients.
 * ppgat_gemm_nn:  y[m, n] = alpha x[m, k] B + bias  with B[k][j] = b[k * ldb + j] (b_layout 0)
 *                 or b[j * ldb + k] (b_layout 1: x W^T with W = b [n, k]); k % 32 == 0,
 *                 n % 128 == 0; bias nullable.
 * ppgat_gemm_tn_big: out[ma, nb] = a[m, ma]^T b[m, nb] over m rows, ma and nb multiples of 128;
 *                 row splits summed in split order (deterministic); workspace queried first.
 * ppgat_colsum:   out[c] = sum_i y[i, c] (c in {128, 256}), fixed order. */
int ppgat_gemm_nn_supported(int64_t m, int k, int n, int b_layout);
int ppgat_gemm_nn(const float* x, int64_t ldx, int64_t m, int k, const float* b, int64_t ldb, int b_layout, int n,
                  float alpha, const float* bias, float* y, int64_t ldy, void* stream);
/* ppgat_gemm_nn_ws: the same product; with few output tiles (small m, e.g. a 512-row batch)
 *   and a long reduction it splits k over workgroups into the workspace and sums the splits in
 *   order (deterministic); workspace_bytes() returns 0 when no split is taken. */
int ppgat_gemm_nn_workspace_bytes(int64_t m, int k, int n, size_t* bytes);
int ppgat_gemm_nn_ws(const float* x, int64_t ldx, int64_t m, int k, const float* b, int64_t ldb, int b_layout, int n,
                     float alpha, const float* bias, float* y, int64_t ldy, void* workspace, size_t workspace_bytes,
                     void* stream);
/* ppgat_gemm_nn_rank: y = alpha x b + bias + s a (s [m, nv] with row stride lds, a [nv, n] with
 *   row stride lda, nv <= 16, the terms added in v order after alpha and bias: the bits of
 *   ppgat_gemm_nn_ws followed by ppgat_rows_rank_update).  On the fp16 two-term large-m path
 *   with nv <= 8 the rank terms are added in the GEMM's epilogue (no second pass over y) --
 *   the multi-head backward's dx = acc W / H + S A_att (ppgat_xgat_bwd_edges_g).  Same
 *   workspace as ppgat_gemm_nn_ws. */
int ppgat_gemm_nn_rank(const float* x, int64_t ldx, int64_t m, int k, const float* b, int64_t ldb, int b_layout, int n,
                       float alpha, const float* bias, const float* s, int64_t lds, int nv, const float* a,
                       int64_t lda, float* y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream);
int ppgat_gemm_tn_big_workspace_bytes(int64_t m, int ma, int nb, size_t* bytes);
int ppgat_gemm_tn_big(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t m, int ma, int nb, float* out,
                      void* workspace, size_t workspace_bytes, void* stream);
/* ppgat_gemm_tn_big_bounded: the same product, with the caller's upper bound of |b| per column
 *   (b_bound_bits[j % bound_period] as IEEE bits, times bound_scale >= 1) in place of the
 *   column-max pass over b that the fp16 two-term kernel otherwise makes -- e.g. the multi-head
 *   layer's G = g^T agg with |agg^h_i[k]| <= max_j |x_j[k]| / (1 - p) (train_gat_pyg.py:77 backward).
 *   The fp16 split's error is relative to the bound, not to b's own column maxima: a column
 *   whose bound is 2^k above its true maximum loses about k bits (22 - k significant bits per
 *   product), so the bound should be tight -- for agg, the column maxima over the rows that are
 *   the SOURCE of an edge (ppgat_colmax_abs_sources), not over all rows of x.  The fp32 / bf16
 *   families ignore it.
 * ppgat_colmax_abs: out_bits[c] = IEEE bits of max_i |x[i, c]| (order-free: deterministic).
 * ppgat_colmax_abs_sources: the same over the rows i with src_ptr[i + 1] > src_ptr[i] (src_ptr:
 *   the CSC pointers [n + 1] of the edge list; rows with no out-edge never enter an aggregate). */
int ppgat_gemm_tn_big_bounded(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t m, int ma, int nb,
                              const unsigned* b_bound_bits, int bound_period, float bound_scale, float* out,
                              void* workspace, size_t workspace_bytes, void* stream);
/* ppgat_gemm_tn_big_bounds: both bounds the caller's (either nullable: that operand's column-max
 *   pass instead).  a_bound_bits[i] bounds |a[r, i]| over the rows r whose b row is NOT all zero
 *   (e.g. g over the destinations that have an in-edge, from ppgat_xgat_bwd_edges_gd_colmax, for
 *   G = g^T agg: agg_r = 0 without in-edges); the other rows' a values are clamped to the fp16
 *   range in the split, so they add 0 as they must.  b_bound_bits as in _bounded. */
int ppgat_gemm_tn_big_bounds(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t m, int ma, int nb,
                             const unsigned* a_bound_bits, const unsigned* b_bound_bits, int bound_period,
                             float bound_scale, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* ppgat_gemm_tn_big_colsum: ppgat_gemm_tn_big_bounds (either bound nullable) that also writes
 *   colsum_out[i] = sum_r a[r, i] (the bias gradient beside a weight gradient: Linear.bias,
 *   GATConv.bias) -- on the fp16 TN kernel from the rows its staging threads already hold (no
 *   second pass over a), in a fixed order: deterministic.  Replaces the reference's separate
 *   autograd sum for the bias (torch.nn.Linear / PyG GATConv bias, train_gat_pyg.py:75-77). */
int ppgat_gemm_tn_big_colsum(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t m, int ma, int nb,
                             const unsigned* a_bound_bits, const unsigned* b_bound_bits, int bound_period,
                             float bound_scale, float* out, float* colsum_out, void* workspace,
                             size_t workspace_bytes, void* stream);
int ppgat_colmax_abs(const float* x, int64_t ldx, int64_t n, int c, unsigned* out_bits, void* stream);
int ppgat_colmax_abs_sources(const float* x, int64_t ldx, int64_t n, int c, const int32_t* src_ptr,
                             unsigned* out_bits, void* stream);
int ppgat_colsum_workspace_bytes(int64_t n, int c, size_t* bytes);
int ppgat_colsum(const float* y, int64_t ldy, int64_t n, int c, float* out, void* workspace, size_t workspace_bytes,
                 void* stream);

/* ---- multi-head layer, aggregate-then-transform ----------------------------------------------
 * Replaces: GATConv(C_in, C, heads=H, concat=False) forward and backward (train_gat_pyg.py:77,
 *           SURVEY.md Appendix A) when H*C > C_in -- config 5 (C_in = C = 256, H = 4).  The
 *           message is linear in x_j, so the edge pass gathers x_j (C_in floats) once per edge
 *           for all heads instead of h_j (H*C floats):
 *   att_proj [2, H, C_in]: A_v[h] = W_h^T att_v[h]                      (ppgat_xgat_weights)
 *   w_xform [H*C_in, C]: w_xform[h*C_in + k][c] = W[h*C + c][k];  w_grad [C, H*C_in] = w_xform^T / H
 *   s_src[n][h] = x_n . A_src[h] (n < n_rows), s_dst likewise (n < n_dst)   (ppgat_xgat_scores)
 *   agg[i][h] = sum_{j->i} alpha_ij^h x_j, m, inv_l [n_dst, H]  (ppgat_xgat_fwd; CSR over the
 *     destination rows; x rows indexed by col may extend past n_dst: the halo rows of dist.py)
 *   out = agg w_xform / H + bias                                          (ppgat_gemm_nn)
 * Backward with g = dL/dout: gt = g w_grad [n_dst, H*C_in] (ppgat_gemm_nn); nstate[i][h] =
 * {s_dst, m, inv_l, gt_i^h . agg_i^h} (prologue); one pass by source over the CSC
 * (ppgat_xgat_bwd_edges): dx_j = sum_k sum_h beta gt_i^h + sum_h ds_src_j^h A_src[h],
 * S[j][h] = ds_src, dz at each edge's CSR slot; S[i][H + h] = ds_dst by ppgat_bwd_dst_sum;
 * dx_i += sum_h ds_dst_i^h A_dst[h] (epilogue); GV = S^T x [2H, C_in] (ppgat_gemm_tn),
 * G = g^T agg [C, H*C_in] (ppgat_gemm_tn_big); dW, datt (ppgat_xgat_weight_grads):
 *   dW[h*C + c][k] = G[c][h*C_in + k] / H + att_src[h][c] GV[h][k] + att_dst[h][c] GV[H+h][k],
 *   datt_v[h][c] = sum_k W[h*C + c][k] GV[v*H + h][k].
 * Supported: C_in = 256, H in {2, 4}, C % 128 == 0 (ppgat_xgat_supported).  Dropout as ppgat_fwd
 * (seed_used required when dropout_p > 0: the forward writes it, the backward reads it). */
int ppgat_xgat_supported(int in_channels, int heads, int channels);
int ppgat_xgat_weights(const float* w, const float* att_src, const float* att_dst, int heads, int channels,
                       int in_channels, float* att_proj, float* w_xform, float* w_grad, void* stream);
int ppgat_xgat_scores(const float* x, int64_t ldx, int64_t n_rows, int64_t n_dst, int in_channels, int heads,
                      const float* att_proj, float* s_src, float* s_dst, void* stream);
int ppgat_xgat_fwd_workspace_bytes(int64_t n_hub_items, int heads, int in_channels, size_t* bytes);
int ppgat_xgat_fwd(const ppgat_schedule* dst_sched, const int32_t* col, const int32_t* csr_eid, int64_t n_dst,
                   int64_t n_edges, int in_channels, int heads, const float* x, int64_t ldx, const float* s_src,
                   const float* s_dst, float negative_slope, float dropout_p, uint64_t seed, uint64_t* seed_used,
                   float* agg, float* m, float* inv_l, void* workspace, size_t workspace_bytes, void* stream);
/* ppgat_xgat_fwd that also merges into x_colmax_bits[k] (caller-initialised, e.g. zeros; 16-byte
 * aligned) the IEEE bits of max |x_j[k]| over the rows it gathers -- every source of an edge,
 * the rows ppgat_colmax_abs_sources covers -- by atomic max (order-free: deterministic).  The
 * bound of |agg| the weight gradient's fp16 split needs, without a pass over x. */
int ppgat_xgat_fwd_colmax(const ppgat_schedule* dst_sched, const int32_t* col, const int32_t* csr_eid, int64_t n_dst,
                          int64_t n_edges, int in_channels, int heads, const float* x, int64_t ldx, const float* s_src,
                          const float* s_dst, float negative_slope, float dropout_p, uint64_t seed,
                          uint64_t* seed_used, float* agg, float* m, float* inv_l, unsigned* x_colmax_bits,
                          void* workspace, size_t workspace_bytes, void* stream);
int ppgat_xgat_bwd_prologue(const float* gt, const float* agg, const float* s_dst, const float* m, const float* inv_l,
                            int64_t n_dst, int in_channels, int heads, float* nstate, void* stream);
int ppgat_xgat_bwd_workspace_bytes(int64_t n_hub_items, int in_channels, size_t* bytes);
int ppgat_xgat_bwd_edges(const ppgat_schedule* src_sched, const int32_t* row, const int32_t* csc_eid,
                         const int32_t* dz_slot, int64_t n_edges, int in_channels, int heads, const float* x,
                         int64_t ldx, const float* s_src, const float* nstate, const float* gt, const float* att_proj,
                         float negative_slope, float dropout_p, uint64_t seed, const uint64_t* seed_used, float* dx,
                         int64_t lddx, float* S, int64_t lds, float* dz, void* workspace, size_t workspace_bytes,
                         void* stream);
/* The same backward edge pass gathering g_i (C floats per edge) instead of gt_i (H * C_in):
 *   dalpha^h_ij = g_i . hs^h_j with hs^h_j = W_h x_j / heads (caller's GEMM, [n_src, H, C]),
 *   acc[j][h] = sum_k beta^h g_i [n_src, H, C]; dx = acc W / heads (caller's GEMM, W = lin.weight
 *   [H*C, C_in]) + the attention terms of S (ppgat_gemm_nn_rank).  dz, S[:, :H] as
 *   ppgat_xgat_bwd_edges.  Channels C == 256, heads 2 or 4. */
int ppgat_xgat_bwd_g_workspace_bytes(int64_t n_hub_items, int channels, int heads, size_t* bytes);
int ppgat_xgat_bwd_edges_g(const ppgat_schedule* src_sched, const int32_t* row, const int32_t* csc_eid,
                           const int32_t* dz_slot, int64_t n_edges, int channels, int heads, const float* hs,
                           const float* s_src, const float* nstate, const float* g, int64_t ldg, float negative_slope,
                           float dropout_p, uint64_t seed, const uint64_t* seed_used, float* acc, float* S, int64_t lds,
                           float* dz, void* workspace, size_t workspace_bytes, void* stream);
/* Deferred D (the default multi-head backward: no gt GEMM, no gt.agg prologue).  The prologue's
 * D^h_i = gt^h_i . agg^h_i equals sum_j beta^h_ij dalpha^h_ij with dalpha = g_i . hs^h_j, so:
 *   ppgat_xgat_nstate: nstate[i][h] = {s_dst, m, inv_l, D or 0 (D NULL)}, D [n_dst, heads];
 *   ppgat_xgat_bwd_edges_gd: ppgat_xgat_bwd_edges_g's pass with dalpha and pdalpha = beta dalpha
 *     stored per edge and head (at dz_slot, as dz) instead of dz and ds_src; acc as _g;
 *   D = the destination sum of pdalpha (ppgat_bwd_dst_sum_csc / ppgat_bwd_dst_sum, heads H);
 *   ppgat_xgat_bwd_dz: dz = alpha e'(z) (dm dalpha - D_i) in place over dalpha (by source over
 *     the CSC; nstate with D) and S[j][h] = ds_src_j = sum of the source's dz (fixed order);
 *   ds_dst = the destination sum of dz, as before.  Heads 2 or 4. */
int ppgat_xgat_bwd_edges_gd(const ppgat_schedule* src_sched, const int32_t* row, const int32_t* csc_eid,
                            const int32_t* dz_slot, int64_t n_edges, int channels, int heads, const float* hs,
                            const float* s_src, const float* nstate, const float* g, int64_t ldg,
                            float negative_slope, float dropout_p, uint64_t seed, const uint64_t* seed_used,
                            float* acc, float* dalpha, float* pdalpha, void* workspace, size_t workspace_bytes,
                            void* stream);
/* ppgat_xgat_bwd_edges_gd that also merges into g_colmax_bits[c] the bits of max |g_i[c]| over the
 * rows it gathers (every destination of an edge), as ppgat_xgat_fwd_colmax: the A bound of
 * ppgat_gemm_tn_big_bounds for G = g^T agg. */
int ppgat_xgat_bwd_edges_gd_colmax(const ppgat_schedule* src_sched, const int32_t* row, const int32_t* csc_eid,
                                   const int32_t* dz_slot, int64_t n_edges, int channels, int heads, const float* hs,
                                   const float* s_src, const float* nstate, const float* g, int64_t ldg,
                                   float negative_slope, float dropout_p, uint64_t seed, const uint64_t* seed_used,
                                   float* acc, float* dalpha, float* pdalpha, unsigned* g_colmax_bits,
                                   void* workspace, size_t workspace_bytes, void* stream);
int ppgat_xgat_nstate(const float* s_dst, const float* m, const float* inv_l, const float* D, int64_t n_dst, int heads,
                      float* nstate, void* stream);
/* Halo partition (dist.py): set the D component of every row of an nstate table whose other three
 * came by exchange -- nstate[i][h].w = D[i * heads + h] for i < n_rows.  Replaces dist.py:
 * `ntab.x.view(R, H, 4)[:, :, 3].copy_(Dtab.x)` (no reference counterpart: the reference has no
 * sharded backward). */
int ppgat_xgat_nstate_set_d(float* nstate, const float* D, int64_t n_rows, int heads, void* stream);
int ppgat_xgat_bwd_dz_workspace_bytes(int64_t n_hub_items, int heads, size_t* bytes);
int ppgat_xgat_bwd_dz(const ppgat_schedule* src_sched, const int32_t* row, const int32_t* csc_eid,
                      const int32_t* dz_slot, int64_t n_edges, int heads, const float* s_src, const float* nstate,
                      float negative_slope, float dropout_p, uint64_t seed, const uint64_t* seed_used, float* dz,
                      float* S, int64_t lds, void* workspace, size_t workspace_bytes, void* stream);
int ppgat_xgat_bwd_epilogue(const float* S, int64_t lds, const float* att_proj, int64_t n_dst, int in_channels,
                            int heads, float* dx, int64_t lddx, void* stream);
int ppgat_xgat_weight_grads(const float* G, const float* GV, const float* w, const float* att_src,
                            const float* att_dst, int heads, int channels, int in_channels, float* dW, float* datt_src,
                            float* datt_dst, void* stream);

/* ---- multi-head layer, transform-then-aggregate (H*C <= C_in, or the replicated partition) ----
 * Replaces: the input-gradient terms of GATConv's attention logits (PyG, train_gat_pyg.py:77;
 *   SURVEY.md Appendix B): dx = D W + ds_src A_src + ds_dst A_dst, with D W on ppgat_gemm_nn.
 * ppgat_att_proj: att_proj [2, H, C_in] = [W_h^T att_src[h]; W_h^T att_dst[h]] for any shape
 *   (W [H*C, C_in] row-major, att [H, C]).
 * ppgat_rows_rank_update: dx[i][k] += sum_{v < nv} S[i][v] A[v][k] (v ascending) over n_rows
 *   rows, nv <= 16, k % 4 == 0, 16-byte aligned A / dx rows.  Deterministic. */
int ppgat_att_proj(const float* w, const float* att_src, const float* att_dst, int heads, int channels,
                   int in_channels, float* att_proj, void* stream);
int ppgat_rows_rank_update(const float* S, int64_t lds, int nv, const float* A, int64_t lda, int64_t n_rows, int k,
                           float* dx, int64_t lddx, void* stream);

/* ---- validation / debug build -----------------------------------------------------------
 * ppgat_check_index_range: *n_bad = number of entries of idx (int32 when elem_bytes == 4,
 *   int64 when 8) outside [lo, hi); synchronises the stream (a validation tool, not for use
 *   inside a captured graph).  Used by the Python layer to validate graph views and exchange
 *   plans when the library is a debug build.
 * ppgat_debug_build: 1 for libppgat_debug.so (make debug: -O1 -g -DPPGAT_DEBUG=1), whose entry
 *   points validate the index inputs whose bounds they know (BPR triples, eval users and
 *   candidates, serving histories) and synchronise after their kernels, so an asynchronous
 *   fault is reported by the entry point that launched it; 0 for libppgat.so. */
int ppgat_debug_build(void);
int ppgat_check_index_range(const void* idx, int elem_bytes, int64_t n, int64_t lo, int64_t hi, int64_t* n_bad,
                            void* stream);

/* ---- measurement ------------------------------------------------------------------------
 * ppgat_stream_copy: dst[0 .. n_bytes) = src[...], a float4 streaming copy (16 B per lane,
 *   non-temporal loads and stores, one pass): the achievable-HBM yardstick bench.py reports
 *   beside the 8 TB/s spec peak (the guide's measured float4 copy: 6.29 TB/s; this one 6.58 on
 *   1 GiB, profiles/r06/x3_copy_lab.log).  n_bytes and both pointers must be multiples of 16. */
int ppgat_stream_copy(const void* src, void* dst, int64_t n_bytes, void* stream);

/* ---- in-process kernel timing (HIP events on the launch stream) --------- */
#define PPGAT_K_CSR 0
#define PPGAT_K_SCORES 1
#define PPGAT_K_FWD 2
#define PPGAT_K_BWD_PRO 3
#define PPGAT_K_BWD_SRC 4
#define PPGAT_K_BWD_EPI 5
#define PPGAT_K_BWD_RED 6
#define PPGAT_K_SCHED 7
#define PPGAT_K_GEMM_TN 8
#define PPGAT_K_FUSION 9
#define PPGAT_K_PROJ 10
#define PPGAT_K_ADAM 11
#define PPGAT_K_SAMPLE 12
#define PPGAT_K_INFONCE 13
#define PPGAT_K_PROJ_BWD 14
#define PPGAT_K_COUNT 15
int ppgat_profile_enable(int on);
int ppgat_profile_reset(void);
/* Synchronises the recorded events; total milliseconds and launch count of kernel k. */
int ppgat_profile_read(int kernel, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* PPGAT_H */
