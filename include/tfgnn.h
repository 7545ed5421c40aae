/*
 * tfgnn.h - C ABI of the MI355X-native (gfx950) message-passing hot path of microsoft/tf2-gnn.
 *
 * The reference (/root/reference, pure Python on TensorFlow 2) has no FFI of its own: every
 * "kernel" on its hot path is a stock TensorFlow op dispatched from
 * tf2_gnn/layers/message_passing/{message_passing,gnn_edge_mlp,rgcn,rgin,ggnn,rgat}.py and tf2_gnn/layers/nodes_to_graph_representation.py.
 * This header therefore declares one entry point per TensorFlow op (or fused group of ops) that
 * path dispatches; each declaration cites the reference call site it replaces (file:line relative
 * to /root/reference).  A maintainer binds them with ctypes.
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer (HIP), row-major, contiguous unless a leading
 *     dimension (ld*, counted in elements) is given; floats are IEEE fp32, indices int32.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued on it,
 *     no entry point synchronises except tfgnn_graph_create (one small D2H validity read).
 *   - return value: 0 on success, negative tfgnn_status otherwise; tfgnn_last_error() returns a
 *     thread-local description of the last failure.
 *   - inputs are never written; outputs must not alias inputs unless stated.
 */
#ifndef TFGNN_H
#define TFGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  TFGNN_OK = 0,
  TFGNN_ERR_INVALID_ARGUMENT = -1, /* bad shape / null pointer / unknown enum           */
  TFGNN_ERR_OUT_OF_RANGE = -2,     /* node index outside [0, V) (TF Gather: InvalidArgument) */
  TFGNN_ERR_HIP = -3,              /* a HIP runtime call failed                          */
  TFGNN_ERR_UNSUPPORTED = -4
} tfgnn_status;

/* tf2_gnn/utils/param_helpers.py:25-33 (+ "none" = identity, "sigmoid" for pooling weights,
 * nodes_to_graph_representation.py:176) */
typedef enum {
  TFGNN_ACT_NONE = 0,
  TFGNN_ACT_RELU = 1,
  TFGNN_ACT_TANH = 2,
  TFGNN_ACT_LEAKY_RELU = 3, /* alpha = 0.2 (tf.nn.leaky_relu default) */
  TFGNN_ACT_ELU = 4,
  TFGNN_ACT_SELU = 5,
  TFGNN_ACT_GELU = 6, /* tanh approximation, tf2_gnn/utils/activation.py:7-14 */
  TFGNN_ACT_SIGMOID = 7
} tfgnn_activation;

/* tf2_gnn/utils/param_helpers.py:9-14 */
typedef enum {
  TFGNN_REDUCE_SUM = 0,
  TFGNN_REDUCE_MAX = 1 /* empty segment -> lowest finite float, like tf.math.unsorted_segment_max */
} tfgnn_reduce;

const char* tfgnn_last_error(void);
/* "tfgnn <version> gfx950" */
const char* tfgnn_version(void);
/* Bumped whenever an existing entry point changes its signature or meaning (round 4: 2 - tfgnn_gemm_grad_epilogue gained
 * `accumulate` in round 3, tfgnn_gemm_get_mode can return TFGNN_GEMM_F16X2, the bucketing keeps list order inside a bucket).
 * 5: tfgnn_sp_gemm_tn_wide lost its job argument, the layer-level argument structs lost their pending-job fields, and four
 * entry points of rejected variants (staged weight-gradient products, a batched weight split) were removed.
 * A binding compares tfgnn_abi_version() with the TFGNN_ABI_VERSION it was written against (tf2_gnn_amd/_lib.py does). */
#define TFGNN_ABI_VERSION 5
int tfgnn_abi_version(void);

/* Diagnostics (no reference counterpart): number of launches of each product-kernel family this process has enqueued
 * since the library was loaded - host-side counters, no device work.  The parity tests read them around a layer call
 * to assert that a GEMM mode (tfgnn_gemm_set_mode / the f16x2 layer paths) really ran the kernels it names, so that
 * parity evidence and timing evidence are about the same code. */
typedef enum {
  TFGNN_KFAM_GEMM_FP32 = 0,   /* gemm_mfma_kernel (v_mfma_f32_32x32x2_f32)                       */
  TFGNN_KFAM_GEMM_BF16X3 = 1, /* gemm_x3s / gemm_x3p kernels (3-way bf16 split inside the GEMM)    */
  TFGNN_KFAM_SP_NT = 2,       /* gemm_sp_nt_kernel (pre-split fp16 pairs, forward / input gradient) */
  TFGNN_KFAM_SP_TN = 3,       /* gemm_sp_tn_kernel (pre-split fp16 pairs, weight gradient)          */
  TFGNN_KFAM_GATHER_SP = 4,   /* csr_gather_reduce_kernel writing the SP16 operand                  */
  TFGNN_KFAM_GATHER = 5,      /* csr_gather_reduce_kernel, fp32 output                              */
  TFGNN_KFAM_FUSED_NT = 6,    /* reserved (the gather-producing product was measured and not shipped) */
  TFGNN_KFAM_GEMM_STREAM = 7, /* gemm_x3k_kernel: bf16x3 products with the weight block resident in LDS (short K,
                                 very many rows); every such launch also counts as TFGNN_KFAM_GEMM_BF16X3 */
  TFGNN_KFAM_STREAM_F16X2 = 8, /* gemm_x3k_kernel in the f16x2 arithmetic (round 6: mode f16x2; 3 products, operands split on the fly);
                                  such a launch counts here and as TFGNN_KFAM_GEMM_STREAM, NOT as TFGNN_KFAM_GEMM_BF16X3 */
  TFGNN_KFAM_COUNT = 9
} tfgnn_kernel_family;
int tfgnn_launch_counts(int64_t* out_counts, int n);

/* ------------------------------------------------------------------------------------------
 * Graph handle: the (dst, edge_type)- and (src, edge_type)-bucketed adjacency of one batch.
 * Replaces, for all L layers and both passes of a step, the per-layer work of
 *   message_passing.py:195-206 (slicing src/dst columns, embedding_lookup of the degree),
 *   message_passing.py:230-263 calculate_type_to_num_incoming_edges (scatter_nd of ones),
 *   message_passing.py:166-167 (concat of targets / messages over edge types).
 * Row r = node * L + edge_type.  Within a row, columns ascend (canonical, deterministic).
 * ------------------------------------------------------------------------------------------ */
typedef struct tfgnn_graph tfgnn_graph;

/* d_adjacency[l] : device int32 [num_edges[l], 2], row k = (source, target)  (gnn.py:241-244).
 * The array of pointers and num_edges live on the HOST. */
int tfgnn_graph_create(int num_edge_types, int64_t num_nodes, const int32_t* const* d_adjacency,
                       const int64_t* num_edges, void* stream, tfgnn_graph** out_graph);
int tfgnn_graph_destroy(tfgnn_graph* graph);
/* Pipelined form (the reference prepares batches in a background thread + tf.data prefetch,
 * data/graph_dataset.py:292-295, cli_utils/training_utils.py:114-115): enqueue the whole build on
 * `stream` and return at once; tfgnn_graph_wait blocks the HOST until the build has finished, then
 * reports bad indices.  Consumers on other streams must order themselves after `stream` (event /
 * stream wait) and call tfgnn_graph_wait before the first gather.  tfgnn_graph_destroy_async returns
 * the handle's memory to the library's pool, to be reused only after the work already enqueued on
 * `last_use_stream` (tfgnn_graph_destroy waits for the device instead). */
int tfgnn_graph_create_async(int num_edge_types, int64_t num_nodes, const int32_t* const* d_adjacency,
                             const int64_t* num_edges, void* stream, tfgnn_graph** out_graph);
int tfgnn_graph_wait(tfgnn_graph* graph);
int tfgnn_graph_destroy_async(tfgnn_graph* graph, void* last_use_stream);

/* What a batch's handle holds beyond the two sorted edge orders (row pointers, columns, edge ids, degrees: always built).
 * A layer stack that only runs the aggregate-first RGCN / GGNN path needs the typed plans alone; everything else costs
 * preparation kernels per batch for arrays nobody reads.  tfgnn_graph_create / _async build everything (as before);
 * tfgnn_graph_create_parts_async builds the requested parts; tfgnn_graph_ensure adds missing ones later on `stream`
 * (it blocks the host: the sizes of a part come back from the device).  Entry points that need a part the handle does
 * not have fail with TFGNN_ERR_INVALID_ARGUMENT and name the part - they never read unbuilt arrays.
 * LIFETIME / ORDERING of tfgnn_graph_ensure(EDGE_IDS | EDGE_MAPS) on a handle created without EDGE_IDS: it sorts again - it
 * reads the adjacency lists of the creation call a second time (the caller must still own them) and REWRITES the handle's
 * row pointers / columns / degrees in place with identical values, on `stream`.  Kernels reading the handle on ANOTHER
 * stream at that moment race with those writes: call it only from the stream that uses the handle, or - better - name the
 * parts at creation (a stack with RGAT or per-edge messages: EDGE_MAPS / EDGE_IDS; tf2_gnn_amd: GNN.graph_parts does). */
typedef enum {
  TFGNN_GRAPH_PART_PLAN_TYPED = 1, /* long-row plans + length-ordered short rows of the views BY_DST_TYPED / BY_SRC_TYPED */
  TFGNN_GRAPH_PART_PLAN_NODE = 2,  /* ... of the views BY_DST_NODE / BY_SRC_NODE (RGAT, per-edge messages)                */
  TFGNN_GRAPH_PART_COMPACT = 4,    /* non-empty (node, type) buckets, type-major: TFGNN_G_NZ_* and the COMPACT views        */
  TFGNN_GRAPH_PART_EDGE_MAPS = 8,  /* TFGNN_G_SRC2DST_POS and its inverse (RGAT: attention weights in both edge orders);
                                      implies EDGE_IDS                                                                      */
  TFGNN_GRAPH_PART_EDGE_IDS = 16,  /* TFGNN_G_EID_BY_DST / _SRC: the position of every bucketed edge in the caller's lists
                                      (per-edge message forms).  Without it the sort moves 4 bytes per edge and digit instead
                                      of 8.  Added later by tfgnn_graph_ensure it costs a second sort, which READS THE
                                      ADJACENCY LISTS OF THE CREATION CALL AGAIN: keep them alive.                          */
  TFGNN_GRAPH_PART_DST_PATTERN = 32, /* TFGNN_G_PATTERN_*: the nodes ordered by which of their by-target buckets are empty, and per
                                      128 positions the union of those patterns - lets the forward product of the aggregate-first
                                      layers skip the all-zero K blocks of a row tile (TFGNN_VIEW_BY_DST_TYPED_PATTERN, the tile
                                      mask / row map arguments of tfgnn_sp_gemm_nt_dropout); at most 8 edge types, empty beyond  */
  TFGNN_GRAPH_PARTS_DEFAULT = 31, /* what tfgnn_graph_create_async builds: everything but the pattern order (on request) */
  TFGNN_GRAPH_PARTS_ALL = 63
} tfgnn_graph_part;
int tfgnn_graph_create_parts_async(int num_edge_types, int64_t num_nodes, const int32_t* const* d_adjacency,
                                   const int64_t* num_edges, unsigned parts, void* stream, tfgnn_graph** out_graph);
int tfgnn_graph_ensure(tfgnn_graph* graph, unsigned parts, void* stream);
unsigned tfgnn_graph_parts(const tfgnn_graph* graph);

typedef enum {
  TFGNN_G_ROWPTR_BY_DST = 0, /* int32 [V*L+1]                                                  */
  TFGNN_G_COL_BY_DST = 1,    /* int32 [E]  source node of each bucketed edge                  */
  TFGNN_G_EID_BY_DST = 2,    /* int32 [E]  position of the edge in concat(adjacency_lists)    */
  TFGNN_G_COLL_BY_DST = 3,   /* int32 [E]  source * L + edge_type (row of a [V*L, H] tensor)  */
  TFGNN_G_ROWPTR_BY_SRC = 4, /* int32 [V*L+1]                                                  */
  TFGNN_G_COL_BY_SRC = 5,    /* int32 [E]  target node                                        */
  TFGNN_G_EID_BY_SRC = 6,    /* int32 [E]                                                     */
  TFGNN_G_COLL_BY_SRC = 7,   /* int32 [E]  target * L + edge_type                             */
  TFGNN_G_INVDEG_BY_DST = 8, /* float [V*L] 1/(in_degree[l,v] + 1e-7) (gnn_edge_mlp.py:102-106), 0 for empty rows */
  TFGNN_G_INVDEG_EDGE_BY_SRC = 9, /* float [E] same quantity per edge, in by-src order        */
  TFGNN_G_NODEPTR_BY_DST = 10,    /* int32 [V+1] = ROWPTR_BY_DST[::L] (all edge types of a target) */
  TFGNN_G_NODEPTR_BY_SRC = 11,    /* int32 [V+1]                                               */
  TFGNN_G_INVDEG_EDGE_BY_DST = 12, /* float [E] per edge, by-dst order                          */
  TFGNN_G_SRC2DST_POS = 13,       /* int32 [E] position in by-dst order of the edge at each by-src position */
  TFGNN_G_TARGET_BY_DST = 14,     /* int32 [E] target node of each bucketed edge, by-dst order */
  /* non-empty buckets in type-major order (compact index c): the per-relation multiply only has to
   * visit buckets that received at least one edge (45 % of the (node,type) buckets of an R-MAT batch
   * are empty) */
  TFGNN_G_NZ_CPOS_BY_DST = 15,    /* int32 [V*L] bucket row -> compact index or -1            */
  TFGNN_G_NZ_ROW_BY_DST = 16,     /* int32 [nz]  compact index -> bucket row                  */
  TFGNN_G_NZ_NODE_BY_DST = 17,    /* int32 [nz]  compact index -> node                        */
  TFGNN_G_NZ_OFF_BY_DST = 18,     /* int32 [L+1] first compact index of each edge type        */
  TFGNN_G_NZ_NODEPTR_BY_DST = 19, /* int32 [V+1] CSR over nodes of their non-empty buckets    */
  TFGNN_G_NZ_COL_BY_DST = 20,     /* int32 [nz]  compact indices grouped by node              */
  TFGNN_G_NZ_CPOS_BY_SRC = 21,
  TFGNN_G_NZ_ROW_BY_SRC = 22,
  TFGNN_G_NZ_NODE_BY_SRC = 23,
  TFGNN_G_NZ_OFF_BY_SRC = 24,
  TFGNN_G_NZ_NODEPTR_BY_SRC = 25,
  TFGNN_G_NZ_COL_BY_SRC = 26,
  /* part DST_PATTERN (at most 8 edge types; count 0 beyond): nodes ordered by the emptiness pattern of their by-target buckets */
  TFGNN_G_PATTERN_POS_BY_DST = 27,      /* int32 [V]: node -> position                                  */
  TFGNN_G_PATTERN_NODE_BY_DST = 28,     /* int32 [V]: position -> node (the row map of a product's output) */
  TFGNN_G_PATTERN_TILEMASK_BY_DST = 29, /* uint8 [ceil(V/128)]: union of the patterns of 128 positions (bit l: type l non-empty) */
  /* the same order for the by-SOURCE buckets (also part DST_PATTERN; round 5): the input-gradient product over the by-source
   * sums reads its operand rows through NODE_BY_SRC (tfgnn_sp_gemm_nt_rows d_a_rows) and skips a tile's all-zero blocks */
  TFGNN_G_PATTERN_NODE_BY_SRC = 30,     /* int32 [V]: position -> node */
  TFGNN_G_PATTERN_TILEMASK_BY_SRC = 31, /* uint8 [ceil(V/128)] */
  /* debugging aid: the arrival counters of the gathers over view v = id - 32 (tfgnn_graph_view 0 - 3), int32
   * [multi-item rows of the view's plan x 8]; every entry is 0 whenever no gather over that view is in flight */
  TFGNN_G_GATHER_ARRIVALS_VIEW0 = 32
} tfgnn_graph_array_id;

/* Borrow a device array owned by the handle (valid until tfgnn_graph_destroy). */
int tfgnn_graph_array(const tfgnn_graph* graph, int array_id, const void** d_ptr, int64_t* count);
/* host copy of TFGNN_G_NZ_OFF_* ([L+1] int32; offsets[L] = number of non-empty buckets) */
int tfgnn_graph_nonempty_offsets(const tfgnn_graph* graph, int by_src, int32_t* h_offsets);
int tfgnn_graph_dims(const tfgnn_graph* graph, int64_t* num_nodes, int* num_edge_types,
                     int64_t* num_edges);

/* Scales that fold the degree normalisation (gnn_edge_mlp.py:102-106) and the mean / sqrt_n
 * aggregators (utils/param_helpers.py:12-13) into the gather kernel.
 *   aggregation_mode 0 = sum, 1 = mean (1/max(N_v,1)), 2 = sqrt_n (1/sqrt(max(N_v,1))), N_v = number
 *   of messages entering v over all edge types.
 *   d_row_scale [V*L]          per bucket (v,l): (normalize ? 1/(c_lv+1e-7) : 1) * m_v
 *   d_node_scale [V]           m_v
 *   d_edge_weight_by_src [E]   per edge in by-src order: (normalize ? 1/(c_{l,tgt}+1e-7) : 1) * m_tgt
 *   d_edge_weight_by_dst [E]   per edge in by-dst order: (normalize ? 1/(c_{l,tgt}+1e-7) : 1)          */
int tfgnn_graph_scales(const tfgnn_graph* graph, int normalize_by_num_incoming, int aggregation_mode,
                       float* d_row_scale, float* d_node_scale, float* d_edge_weight_by_src,
                       float* d_edge_weight_by_dst, void* stream);

/* The same three per-node / per-edge arrays for ONE TRAINING STEP WITH EDGE DROPOUT (Schlichtkrull et al. 2018, section 5.2:
 * edges are dropped "before normalization", per layer and per step; DropEdge, Rong et al. 2020).  The layers that read the
 * graph through these arrays alone (RGCN_Basis, RGCN_BlockDiag: tfgnn_basis_gather_*, tfgnn_blockdiag_*) take them in place
 * of tfgnn_graph_scales' and change in nothing else; there is no row scale.
 *   keep      the edge at position e of concat(adjacency_lists) - the id TFGNN_G_EID_BY_DST / _BY_SRC carry - of type l is
 *             KEPT iff element e of the mask tfgnn_dropout_forward draws for (seed, d_rates[l]) at the current dropout epoch
 *             is non-zero ("The dropout mask generator" below: the same key words, hash and epoch step; the threshold
 *             ceil((double)rate * 2^24) is derived on the device from the float32 d_rates[l]).  The decision hangs on e, so
 *             it is the same in both edge orders; rate 0 keeps every edge of the type.  d_rates [L] is DEVICE memory: the
 *             entry reads nothing from the host.  A rate outside [0, 1) cannot be refused without a read-back and is
 *             clamped: below 0 or NaN counts as 0, 1 or more drops every edge of the type.
 *   counts    c'_{v,l} = kept edges of type l into v, N'_v = sum_l c'_{v,l} (integers).
 *   d_node_scale [V]           m_v: mode 0: 1; mode 1: 1.f / max(N'_v, 1); mode 2: 1.f / sqrtf(max(N'_v, 1))
 *   d_edge_weight_by_dst [E]   s_e: 0 for a dropped edge; for a kept one 1.f / ((float)c'_{v,l} + 1e-7f) with normalize, else
 *                              1 in modes 1 and 2 (the kept count inside m_v divides), else - mode 0, a plain sum in which no
 *                              count divides - the inverted-dropout factor 1.f / (1.f - d_rates[l]) of tfgnn_dropout_forward
 *   d_edge_weight_by_src [E]   s'_e = s_e * m_target of the same edge, at its by-source position
 * Where a count divides, it is the count of KEPT edges; where none does, kept edges carry 1 / (1 - p).  The float32
 * expressions are tfgnn_graph_scales': with every rate 0 the three arrays equal its outputs bit for bit, and the values on the
 * kept edges equal what tfgnn_graph_scales gives on the graph made of the kept edges.  A bucket or a node that lost every
 * edge holds zeros / m_v = 1: no NaN, no Inf.
 * Needs part EDGE_MAPS (the inverse of TFGNN_G_SRC2DST_POS carries s'_e to the by-source order; it implies EDGE_IDS) where
 * E > 0 - tfgnn_graph_ensure it outside a capture.  ONE launch (none when V == 0), one wave per target node over the node's
 * row of the by-target order, 64 edges at a time: no lane walks a row alone, integer counts, no atomics, no workspace, no
 * allocation, no copy, no host synchronisation - capturable; every replay of a captured step reads the epoch word again.
 * Refused before the launch: a NULL graph, an unknown mode, NULL outputs where V or E > 0, NULL d_rates where L > 0, a
 * handle without the part. */
int tfgnn_graph_scales_edge_dropout(const tfgnn_graph* graph, int normalize_by_num_incoming, int aggregation_mode,
                                    const float* d_rates /* [L], device */, uint64_t seed,
                                    float* d_node_scale /* [V] */, float* d_edge_weight_by_src /* [E] */,
                                    float* d_edge_weight_by_dst /* [E] */, void* stream);
/* host-side count of the launches the entry above has enqueued in this process: out[0]; further slots are zero */
int tfgnn_edge_dropout_launch_counts(int64_t* out_counts, int n);

/* Helper for use_target_state_as_input with a linear edge layer (gnn_edge_mlp.py:92-97):
 * sum_e s_e [x_u | x_v] W = (sum_e s_e x_u) W_s + k_{l,v} x_v W_t with k = c_{l,v} * row_scale.
 *   d_k [V*L], d_ident_ptr [V*L+1] = 0..V*L, d_node_of_row [V*L] = r / L                           */
int tfgnn_graph_target_multiplier(const tfgnn_graph* graph, const float* d_row_scale, float* d_k,
                                  int32_t* d_ident_ptr, int32_t* d_node_of_row, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gather + segment reduce over a CSR (the hot kernel):
 *   out[r, :] = post_act( row_scale[r] * REDUCE_{e in [rowptr[r], rowptr[r+1])}
 *                                 pre_act( edge_weight[e] * in[col[e], :] ) )
 * Replaces tf.nn.embedding_lookup (message_passing.py:197-206) fused with
 * tf.math.unsorted_segment_{sum,max,mean,sqrt_n} (utils/param_helpers.py:9-14 via
 * message_passing.py:172-174) and the per-message 1/(c+1e-7) scaling (gnn_edge_mlp.py:102-106);
 * mean / sqrt_n are SUM with a row_scale.  d_edge_weight and d_row_scale may be NULL (= 1).
 * width = number of floats per row; ld_in / ld_out = row strides in floats.
 * ------------------------------------------------------------------------------------------ */
int tfgnn_csr_gather_reduce(const int32_t* d_rowptr, const int32_t* d_col,
                            const float* d_edge_weight, const float* d_row_scale,
                            int64_t num_rows, const float* d_in, int64_t ld_in, int width,
                            float* d_out, int64_t ld_out, int reduce_op, int pre_act, int post_act,
                            void* stream);

/* The same reduction over one of the graph handle's four bucketed views, with the handle's plan for
 * long rows (rows with more than 32 edges are cut into 512-edge items, one workgroup each; the partial sums of a row
 * made of several items are added in item order by the item workgroup of the row that finishes last, inside the same
 * launch) - the form the layers use:
 *   TFGNN_VIEW_BY_DST_TYPED  rows (v,l) -> col = source             (aggregate-first forward)
 *   TFGNN_VIEW_BY_DST_NODE   rows v     -> col = source*L + type    (transform-first forward, RGAT)
 *   TFGNN_VIEW_BY_SRC_TYPED  rows (u,l) -> col = target             (backward: scatter by source)
 *   TFGNN_VIEW_BY_SRC_NODE   rows u     -> col = target*L + type
 * d_col_override (nullable) replaces the view's column array (same edge order).  d_edge_weight is
 * [E] (ew_heads == 1) or [E, ew_heads] applied per head of width/ew_heads floats (RGAT attention,
 * rgat.py:154-160).  d_workspace must hold tfgnn_graph_gather_workspace_bytes(graph, view, width).
 * CONCURRENCY: the item workgroups of a long row count their arrivals in the handle (one counter set per view 0 - 3; views
 * 4 - 6 use the counters of the typed view they are made of).  Two gathers over the same view of the same handle must
 * therefore not be in flight at once on different streams; gathers on one stream, over different views, or over
 * different handles need no care.  This holds for every tfgnn_graph_gather_* function and for tfgnn_mp_forward /
 * tfgnn_mp_backward, which gather over views 0 / 6 and 2. */
typedef enum {
  TFGNN_VIEW_BY_DST_TYPED = 0,
  TFGNN_VIEW_BY_DST_NODE = 1,
  TFGNN_VIEW_BY_SRC_TYPED = 2,
  TFGNN_VIEW_BY_SRC_NODE = 3,
  /* the two typed views with COMPACT output: row c of the output belongs to the c-th non-empty
   * bucket in type-major order (TFGNN_G_NZ_* arrays); empty buckets produce no row (and, since round 5, no work: the
   * launch covers the non-empty buckets only).  tfgnn_graph_gather_reduce_sp takes them too: one operand row and one
   * scale per non-empty bucket */
  TFGNN_VIEW_BY_DST_TYPED_COMPACT = 4,
  TFGNN_VIEW_BY_SRC_TYPED_COMPACT = 5,
  /* the by-target typed view with its output rows in PATTERN order: bucket (v, l) is written at row pos[v] * L + l
   * (TFGNN_G_PATTERN_POS_BY_DST), every bucket has a row (part DST_PATTERN) */
  TFGNN_VIEW_BY_DST_TYPED_PATTERN = 6
  /* (7, round 5 only: the same rows without the zero rows of blocks a masked consumer skips - measured no gain, the gather's
   *  time is its reads; removed in round 6 with ABI version 4) */
} tfgnn_graph_view;
size_t tfgnn_graph_gather_workspace_bytes(const tfgnn_graph* graph, int view, int width);
int tfgnn_graph_gather_reduce(const tfgnn_graph* graph, int view, const int32_t* d_col_override,
                              const float* d_edge_weight, int ew_heads, const float* d_row_scale,
                              const float* d_in, int64_t ld_in, int width, float* d_out, int64_t ld_out,
                              int reduce_op, int pre_act, int post_act, void* d_workspace,
                              size_t workspace_bytes, void* stream);

/* Per-edge pieces of GNN_Edge_MLP with target states AND hidden layers (gnn_edge_mlp.py:92-100): the
 * first Dense is separable, [x_u|x_v] W = x_u W_s + x_v W_t, computed per node; per edge only
 *   out[e,:] = act( P[index_a[e],:] + Q[index_b[e],:] )
 * remains.  tfgnn_graph_original_order gives, in the order of the concatenated adjacency lists
 * (type-contiguous, so later Dense layers are GEMMs over [E_l, H] blocks): source*L+type, target*L+type,
 * target node, and (optional) a per-edge weight array re-ordered from by-dst order. */
int tfgnn_edge_pair_combine(const int32_t* d_index_a, const int32_t* d_index_b, const float* d_P,
                            const float* d_Q, int64_t num_edges, int width, int act, float* d_out,
                            void* stream);

/* GNN_FiLM in its per-edge form (gnn_film.py:83-108), for the configurations whose modulated messages go through a max
 * aggregation or a per-message activation (sums are modulated on the node side: tfgnn_film_combine_*):
 *   out[e,:] = gamma[film_row[e],:] * (weight[e] * msg[msg_row[e],:]) + beta[film_row[e],:]
 * d_film rows are [gamma | beta] of width 2 * width; msg_row NULL = identity, edge_weight NULL = 1.  The backward entry
 * writes per-edge terms: grad_msg [E, width] and grad_film [E, 2 * width]; the caller reduces them over message rows /
 * (target, type) buckets with the gather kernel. */
int tfgnn_film_edge_forward(const float* d_msg, const int32_t* d_msg_row, const float* d_film, const int32_t* d_film_row,
                            const float* d_edge_weight, int64_t num_edges, int width, float* d_out, void* stream);
int tfgnn_film_edge_backward(const float* d_grad, const float* d_msg, const int32_t* d_msg_row, const float* d_film,
                             const int32_t* d_film_row, const float* d_edge_weight, int64_t num_edges, int width,
                             float* d_grad_msg, float* d_grad_film, void* stream);

/* Backward through a general aggregation, i.e. the cases the sum-only algebra does not cover:
 * aggregation_function "max" (utils/param_helpers.py:11) and message_activation_before_aggregation
 * (message_passing.py:169-172).  Forward: agg[t,:] = node_scale[t] * REDUCE_{e->t} pre_act(w_e * msg[row_e,:])
 * (tfgnn_graph_gather_reduce).  Per edge, in the order of d_target / d_msg_row / d_edge_weight:
 *   phase 0 (max):  d_out[e,:] = 1 where the edge attains the maximum of its target, else 0
 *                   (segment-sum it to get d_num_selected: TF splits the gradient evenly among ties [ext])
 *   phase 1:        d_out[e,:] = d(loss)/d(msg[row_e,:]) through edge e
 * d_msg_row NULL = identity (messages already per edge); d_agg_max / d_num_selected only for max. */
int tfgnn_edge_aggregate_backward(int64_t num_edges, int64_t width, const float* d_msg, int64_t ld_msg,
                                  const int32_t* d_msg_row, const int32_t* d_target, const float* d_edge_weight,
                                  const float* d_node_scale, int pre_act, int reduce_op, const float* d_grad_agg,
                                  const float* d_agg_max, const float* d_num_selected, int phase, float* d_out,
                                  void* stream);

/* GNN_FiLM (gnn_film.py:84-108): every message is modulated by its target, m' = gamma[l,tgt] * m + beta[l,tgt],
 * with (gamma | beta) = FiLM-MLP_l(h_tgt) [2H].  For sum / mean / sqrt_n aggregation this is a node-side epilogue
 * over the per-bucket message sums Z [V, L, H] (bucket row r = node * L + type):
 *   pre[v,:] = node_scale[v] * sum_l ( film[v,l,:H] * Z[v,l,:] + cnt[v,l] * film[v,l,H:] ),  out = act(pre)
 * cnt[v,l] = d_rowptr_typed[r+1] - d_rowptr_typed[r] (TFGNN_G_ROWPTR_BY_DST).  d_pre may be NULL.
 * Backward: d_grad_pre = d(loss)/d(pre)  ->  d_dZ [V,L,H], d_dfilm [V,L,2H]. */
int tfgnn_film_combine_forward(const float* d_Z, const float* d_film, const int32_t* d_rowptr_typed,
                               const float* d_node_scale, int64_t num_nodes, int num_edge_types, int64_t hidden,
                               int act, float* d_pre, float* d_out, void* stream);
int tfgnn_film_combine_backward(const float* d_grad_pre, const float* d_Z, const float* d_film,
                                const int32_t* d_rowptr_typed, const float* d_node_scale, int64_t num_nodes,
                                int num_edge_types, int64_t hidden, float* d_dZ, float* d_dfilm, void* stream);

/* Batch finalisation of the adjacency lists on the device (tf2_gnn/data/utils.py:9-124, called per batch from
 * data/graph_dataset.py:161-246): the building blocks of process_adjacency_lists.
 *   tfgnn_adjacency_append      d_out[i] = flip ? (dst, src) : (src, dst) of edge i   (_add_backward_edges, :99-113;
 *                               the caller points d_out at the tail of the tied type's list or at a new type's list)
 *   tfgnn_adjacency_self_loops  d_out[i] = (i, i)                                       (_add_self_loop_edges, :88-96)
 *   tfgnn_adjacency_in_degrees  d_counts[v] = number of edges of the list entering v, as float like the reference
 *                               (_compute_type_to_num_inedges, :116-124); targets outside [0, V) are skipped here and
 *                               reported by tfgnn_graph_create
 * Edge lists are int32 [n, 2], 8-byte aligned. */
/* Batching of graph samples into one disjoint-union graph (data/graph_dataset.py:161-246: _add_graph_to_batch shifts
 * graph i's node ids by the nodes before it, :210-222; node_to_graph_map, :211-217; _finalise_batch concatenates).  Per
 * edge type the host lays the graphs' edge lists end to end with their LOCAL node ids (d_local_edges int32 [E, 2]) and
 * passes the prefix sums d_edge_ptr [G+1] (edges of graphs 0..i-1) and d_node_ptr [G+1] (nodes):
 *   tfgnn_batch_offset_edges      d_out[e] = d_local_edges[e] + d_node_ptr[graph of e]; *d_bad_flag (nullable, zeroed by
 *                                 the caller) is set when a local id is outside its graph
 *   tfgnn_batch_node_to_graph_map d_out[v] = graph of node v */
int tfgnn_batch_offset_edges(const int32_t* d_local_edges, int64_t num_edges, const int32_t* d_edge_ptr,
                             const int32_t* d_node_ptr, int num_graphs, int32_t* d_out, int* d_bad_flag, void* stream);
int tfgnn_batch_node_to_graph_map(const int32_t* d_node_ptr, int num_graphs, int64_t num_nodes, int32_t* d_out,
                                  void* stream);
int tfgnn_adjacency_append(const int32_t* d_edges, int64_t num_edges, int flip, int32_t* d_out, void* stream);
int tfgnn_adjacency_self_loops(int64_t num_nodes, int32_t* d_out, void* stream);
int tfgnn_adjacency_in_degrees(const int32_t* d_edges, int64_t num_edges, int64_t num_nodes, float* d_counts,
                               void* stream);
int tfgnn_graph_original_order(const tfgnn_graph* graph, const float* d_weight_by_dst, int32_t* d_src_l,
                               int32_t* d_tgt_l, int32_t* d_tgt_node, float* d_weight, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense layer: C[M,N] = act( op(A)[M,K] @ op(B)[K,N] + bias[N] ) (+ C if accumulate)
 * fp32 in / fp32 accumulate on the matrix cores (v_mfma_f32_32x32x2_f32: exact fp32).
 * Replaces Keras Dense inside dpu_utils MLP (gnn_edge_mlp.py:100, rgin.py:104), rgat.py:102-109,
 * gnn.py:279,324-327, the GRUCell matmuls (ggnn.py:84-87) and their tf.GradientTape gradients
 * (models/graph_task_model.py:347-357).
 *   trans_a = 0: A stored [M,K] (lda >= K);  1: A stored [K,M] (lda >= M)
 *   trans_b = 0: B stored [K,N] (ldb >= N);  1: B stored [N,K] (ldb >= K)
 * d_workspace: scratch for split-K partial sums (may be NULL / 0 -> no split-K).
 * ------------------------------------------------------------------------------------------ */
size_t tfgnn_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int tfgnn_gemm(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const float* d_A,
               int64_t lda, const float* d_B, int64_t ldb, float* d_C, int64_t ldc,
               const float* d_bias, int act, int accumulate, void* d_workspace,
               size_t workspace_bytes, void* stream);

/* How the fp32 products are evaluated (process-wide; initial value from the environment variable
 * TFGNN_GEMM_MODE = fp32 | bf16x3 | bf16x3_9 | f16x2; unset = f16x2, the mode bench.py is timed in):
 *   TFGNN_GEMM_FP32          v_mfma_f32_32x32x2_f32 on the fp32 operands
 *   TFGNN_GEMM_BF16X3        every fp32 operand is split EXACTLY into three bf16 pieces (x = h + m + l) and
 *                            the six largest piece products - each exact in fp32 - are accumulated in fp32 on
 *                            v_mfma_f32_32x32x16_bf16; dropped terms are < 2^-23 |a b| (csrc/gemm_x3.hip)
 *   TFGNN_GEMM_BF16X3_EXACT  all nine piece products: products exact, only the fp32 accumulation rounds
 *   TFGNN_GEMM_F16X2         (default) the products whose operands come out of a kernel that can write them SPLIT (the gather,
 *                            a product's epilogue, the dropout pass) go to the tfgnn_sp_* entry points - operands as two
 *                            rounded fp16 pieces with a power-of-two block scale, 3 piece products ("Split fp16 operands"
 *                            below); the tfgnn_gemm* entry points themselves run as TFGNN_GEMM_BF16X3.  The choice of entry
 *                            point is the binder's: take the tfgnn_sp_* route while tfgnn_gemm_get_mode() returns
 *                            TFGNN_GEMM_F16X2.  The spread guard of the split weight-gradient product
 *                            (tfgnn_sp_spread_flag) demotes the mode inside the library: once it has tripped,
 *                            tfgnn_gemm_get_mode() returns TFGNN_GEMM_BF16X3 until tfgnn_gemm_set_mode(TFGNN_GEMM_F16X2)
 *                            re-arms it (which waits for the device, so that no factor pass in flight can trip it again).
 * Inputs, outputs and accumulators are fp32 in every mode.  The split modes cover N % 128 == 0 (tiles of 320, 256
 * or 128 columns; NN, NT, TN layouts, K >= 64, 16-byte aligned operands); other shapes run the fp32 kernel
 * whatever the mode. */
enum { TFGNN_GEMM_FP32 = 0, TFGNN_GEMM_F16X2 = 3, TFGNN_GEMM_BF16X3 = 6, TFGNN_GEMM_BF16X3_EXACT = 9 };
int tfgnn_gemm_set_mode(int mode);
int tfgnn_gemm_get_mode(void);

/* The input-gradient product with the element-wise factors of the NEXT backward step applied on the way out:
 *   C[M,N] = (op(A) @ op(B)) * mul * act'(saved)      (+ C[M,N] if accumulate: a second term of the same gradient,
 *                                                       e.g. the target half of an edge MLP's concatenated input)
 * mul    = the dropout mask of tf.nn.dropout on the layer input (gnn.py:285-288), NULL = absent;
 * saved  = what tfgnn_activation_backward takes for `act_of_saved` (the activation's output, or its input for
 *          gelu) of the layer below (message_passing.py:176-177 / Dense activation gnn.py:324-327), NULL = absent.
 * Saves two passes over [V, H] per layer boundary.  Returns TFGNN_ERR_UNSUPPORTED when the active GEMM mode / shape
 * has no fused epilogue (only the split-operand NN / NT kernel has one): the caller then runs tfgnn_gemm, tfgnn_mul
 * and tfgnn_activation_backward. */
int tfgnn_gemm_grad_epilogue(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const float* d_A,
                             int64_t lda, const float* d_B, int64_t ldb, float* d_C, int64_t ldc,
                             const float* d_mul, int64_t ld_mul, int act_of_saved, const float* d_saved,
                             int64_t ld_saved, int accumulate, void* d_workspace, size_t workspace_bytes, void* stream);

/* The Dense layer over GATHERED rows: C[m, :] = act( (C[m, :] if accumulate == 2) + A[row_index[m], :] @ op(B) + bias )
 * (+ C[m, :] if accumulate == 1), A [a_rows, lda] fp32, row_index [M] int32 in [0, a_rows); an index outside that range
 * reads as a row of zeros (it never aliases another row).
 * Replaces tf.nn.embedding_lookup(node_embeddings, sources / targets) followed by the first Dense layer of an edge MLP
 * (gnn_edge_mlp.py:84-100 with message_passing.py:195-206): the per-edge input [x_src || x_tgt] W = x_src W_s + x_tgt W_t is
 * two calls (the second with accumulate = 2 and the MLP's activation) and the [E, 2D] concatenation is never written.
 * Only the streaming bf16x3 kernel reads rows through an index (K in {64, 96, 128}, N % 128 == 0, M >= 65536, 16-byte aligned
 * operands, a_rows * lda < 2^30); otherwise TFGNN_ERR_UNSUPPORTED and the caller gathers (tfgnn_gather_reduce with an
 * identity row pointer) and multiplies (tfgnn_gemm) - what the Python mirror does. */
int tfgnn_gemm_gathered(int trans_b, int64_t M, int64_t N, int64_t K, const float* d_A, int64_t lda, int64_t a_rows,
                        const int32_t* d_row_index, const float* d_B, int64_t ldb, float* d_C, int64_t ldc,
                        const float* d_bias, int act, int accumulate, void* stream);
/* 1 if tfgnn_gemm_gathered takes a product of this shape in the current GEMM mode (16-byte aligned operands assumed), else 0:
 * ask before choosing a formulation that only pays with the fused kernel (one message per edge, gnn_edge_mlp.py:84-100). */
int tfgnn_gemm_gathered_supported(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t a_rows);

/* Grouped forms of the Dense layer for the per-relation multiply over NON-EMPTY buckets only (rows of
 * the stacked operand are grouped by edge type: group g owns rows [d_group_offsets[g],
 * d_group_offsets[g+1]), TFGNN_G_NZ_OFF_*; max_group_rows bounds the launch grid):
 *   tfgnn_gemm_grouped_rows: C[rows g] = act( A[rows g] @ op(B + g*stride_b) )   (A [rows,K], B_g [K,N] or [N,K])
 *   tfgnn_gemm_grouped_k:    C + g*stride_c = A[rows g]^T @ B[rows g]             (A [rows,M], B [rows,N]; the
 *                            weight gradient of relation g; split-K with a deterministic second pass) */
int tfgnn_gemm_grouped_rows(int trans_b, int num_groups, const int32_t* d_group_offsets, int64_t max_group_rows,
                            int64_t N, int64_t K, const float* d_A, int64_t lda, const float* d_B, int64_t ldb,
                            int64_t stride_b, float* d_C, int64_t ldc, int act, void* stream);
/* tfgnn_gemm_grouped_rows (act none) times act'(d_saved) - d_saved [rows, N] indexed like C - in the product's epilogue: the
 * input-gradient product of a per-relation MLP layer (gnn_edge_mlp.py:84-100 under tf.GradientTape) with the derivative of the
 * hidden relu below it.  TFGNN_ERR_UNSUPPORTED when the active kernel has no such epilogue (fp32 mode, odd shapes): the
 * caller runs tfgnn_gemm_grouped_rows and tfgnn_activation_backward. */
int tfgnn_gemm_grouped_rows_grad(int trans_b, int num_groups, const int32_t* d_group_offsets, int64_t max_group_rows, int64_t N,
                                 int64_t K, const float* d_A, int64_t lda, const float* d_B, int64_t ldb, int64_t stride_b,
                                 float* d_C, int64_t ldc, int act_of_saved, const float* d_saved, int64_t ld_saved, void* stream);
size_t tfgnn_gemm_grouped_k_workspace_bytes(int num_groups, int64_t max_group_rows, int64_t M, int64_t N);
int tfgnn_gemm_grouped_k(int num_groups, const int32_t* d_group_offsets, int64_t max_group_rows, int64_t M,
                         int64_t N, const float* d_A, int64_t lda, const float* d_B, int64_t ldb, float* d_C,
                         int64_t ldc, int64_t stride_c, void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Element-wise: activations (utils/param_helpers.py:21-39) and their gradients.
 * tfgnn_activation_backward: dx = dy * act'(.) where the derivative is evaluated from the saved
 * OUTPUT y for relu/tanh/leaky_relu/elu/selu/sigmoid and from the saved INPUT x for gelu
 * (pass the matching tensor as d_saved).
 * ------------------------------------------------------------------------------------------ */
int tfgnn_activation_forward(int act, const float* d_x, float* d_y, int64_t n, void* stream);
int tfgnn_activation_backward(int act, const float* d_dy, const float* d_saved, float* d_dx,
                              int64_t n, void* stream);
/* dx = (dy * mul) * act'(saved): tfgnn_mul (the dropout mask of a layer input, gnn.py:285-288) followed by
 * tfgnn_activation_backward (the activation of the layer below) in one pass, bit-equal to the two calls.  16-byte aligned. */
int tfgnn_activation_backward_mul(int act, const float* d_dy, const float* d_saved, const float* d_mul, float* d_dx, int64_t n,
                                  void* stream);

/* ------------------------------------------------------------------------------------------
 * GRUCell gate math ([ext] tf.keras.layers.GRUCell TF2 defaults: reset_after=True, gates z|r|h,
 * sigmoid / tanh), used by GGNN (ggnn.py:64,84-87).  The two matmuls are tfgnn_gemm calls:
 *   mx = x @ kernel + bias[0]   mh = h @ recurrent_kernel + bias[1]      (both [V, 3H])
 * forward:  z = s(mx_z+mh_z), r = s(mx_r+mh_r), c = tanh(mx_h + r*mh_h), h' = z*h + (1-z)*c;
 *           d_gates (nullable) [V,3H] receives z|r|c for the backward pass.
 * backward: d_dmx, d_dmh [V,3H] and d_dh_direct [V,H] = dh' * z.
 * ------------------------------------------------------------------------------------------ */
/* tfgnn_gemm_gru (bf16x3 GEMM modes, H a multiple of 64): the first matmul and the gate math in one kernel -
 *   h' = GRU(mx = x @ kernel + bias[0], mh, h) with mx kept in registers / LDS (never written to HBM).
 * d_kernel_t: the kernel transposed to [3H, K] (K contiguous) with its rows regrouped per block of 192 rows as
 * [z | r | h] of the same 64 units (row t*192 + g*64 + c = column g*H + t*64 + c of the Keras kernel); d_bias
 * (nullable) regrouped likewise.  d_mh as above; d_gates nullable.  TFGNN_ERR_UNSUPPORTED otherwise: callers then
 * use tfgnn_gemm + tfgnn_gru_gates_forward. */
int tfgnn_gemm_gru(int64_t V, int H, int64_t K, const float* d_x, int64_t ld_x, const float* d_kernel_t,
                   const float* d_bias, const float* d_mh, const float* d_h, float* d_h_new, float* d_gates,
                   void* stream);
/* tfgnn_gemm_gru2 (round 6; mode f16x2, H = K in {64, 128}, >= 65536 rows: QM9-sized batches): BOTH products of the cell in the
 * kernel - h' = GRU(x @ kernel + bias[0], h @ recurrent_kernel + bias[1], h) - so that mh [V, 3H] is neither written by a
 * product of its own nor read back.  Both kernels transposed and regrouped as for tfgnn_gemm_gru (d_recurrent_bias likewise,
 * nullable).  d_mh_out (nullable, [V, 3H]): only the candidate third (columns 2H .. 3H) is written - all the backward pass
 * reads of mh (tfgnn_gru_gates_backward*).  TFGNN_ERR_UNSUPPORTED otherwise: callers use tfgnn_gemm + tfgnn_gemm_gru. */
int tfgnn_gemm_gru2(int64_t V, int H, const float* d_x, int64_t ld_x, const float* d_kernel_t, const float* d_bias,
                    const float* d_h, const float* d_recurrent_kernel_t, const float* d_recurrent_bias, float* d_h_new,
                    float* d_gates, float* d_mh_out, void* stream);
int tfgnn_gru_gates_forward(const float* d_mx, const float* d_mh, const float* d_h, float* d_h_new,
                            float* d_gates, int64_t V, int H, void* stream);
int tfgnn_gru_gates_backward(const float* d_dh_new, const float* d_gates, const float* d_mh,
                             const float* d_h, float* d_dmx, float* d_dmh, float* d_dh_direct,
                             int64_t V, int H, void* stream);
/* The same gate gradients for the f16x2 products that consume them (round 3): dmx and dmh [V, 3H] are written ONLY as SP16
 * split operands (one scale per row, d_*_inv_scale [V]) - the operands of tfgnn_sp_gemm_tn (kernel gradients agg^T dmx,
 * h^T dmh) and tfgnn_sp_gemm_nt (d agg = dmx kernel^T, d h += dmh recurrent^T) - and the bias gradients [2, 3H] (column sums
 * of dmx, dmh: fixed-order two-stage reduction) come out of the same pass.  d_out_mul (nullable, [V, H]): an element-wise
 * factor of the state gradient (the dropout mask of the layer's input) applied to d_dh_direct = dh_new * z on the way out.
 * H % 64 == 0, H <= 512 (TFGNN_ERR_UNSUPPORTED otherwise); workspace: tfgnn_gru_gates_backward_sp_workspace_bytes. */
size_t tfgnn_gru_gates_backward_sp_workspace_bytes(int64_t V, int H);
int tfgnn_gru_gates_backward_sp(const float* d_dh_new, const float* d_gates, const float* d_mh, const float* d_h,
                                void* d_dmx_sp, float* d_dmx_inv_scale, void* d_dmh_sp, float* d_dmh_inv_scale,
                                float* d_dh_direct, const float* d_out_mul, float* d_bias_grad, int64_t V, int H,
                                void* d_workspace, size_t workspace_bytes, void* stream);
/* ... with that factor = the mask tfgnn_dropout_forward draws for (dropout_seed, dropout_rate) over the [V, H] layer input,
 * recomputed per element: no mask tensor is read (none exists when the layer input was dropped with d_mask = NULL). */
int tfgnn_gru_gates_backward_sp_dropout(const float* d_dh_new, const float* d_gates, const float* d_mh, const float* d_h,
                                        void* d_dmx_sp, float* d_dmx_inv_scale, void* d_dmh_sp, float* d_dmh_inv_scale,
                                        float* d_dh_direct, float dropout_rate, uint64_t dropout_seed, float* d_bias_grad, int64_t V,
                                        int H, void* d_workspace, size_t workspace_bytes, void* stream);

/* tf.maximum(x, lower) then tf.minimum(., upper) (nodes_to_graph_representation.py:194-197; pass -inf / +inf for an absent
 * bound) and its gradient: dx = dy where lower <= x <= upper, else 0 (TensorFlow's MaximumMinimumGrad).  A NaN in x stays a
 * NaN in y, as in TensorFlow; +-inf clips to the bound (and stays where there is none). */
int tfgnn_clip(const float* d_x, int64_t n, float lower, float upper, float* d_y, void* stream);
int tfgnn_clip_backward(const float* d_dy, const float* d_x, int64_t n, float lower, float upper, float* d_dx, void* stream);
/* out[n] = sum_m in[m, n] (bias gradients of Dense / GRUCell). */
size_t tfgnn_colsum_workspace_bytes(int64_t M, int N);
int tfgnn_colsum(const float* d_in, int64_t M, int N, int64_t ld, float* d_out, void* d_workspace,
                 size_t workspace_bytes, void* stream);
/* out = alpha * (x + y): residual averaging of the layer stack, gnn.py:291-296. */
int tfgnn_add_scale(const float* d_x, const float* d_y, float alpha, float* d_out, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * RGAT (rgat.py:91-163).  Y = X @ [W_0 | ... | W_{L-1}] is a tfgnn_gemm call ([V*L, H] rows (v,l)).
 * tfgnn_rgat_node_scores: the two halves of the attention logit (rgat.py:111-121) per (node,type,head):
 *     s_src[(v,l),k] = <Y[(v,l),k,:], alpha[l,k,:H/K]>   s_tgt[(v,l),k] = <Y[(v,l),k,:], alpha[l,k,H/K:]>
 *     d_alpha: [L, K, 2H/K] (the L "Edge_attention_parameters" stacked, rgat.py:82-86)
 * tfgnn_rgat_edge_scores: score_ek = leaky_relu(s_src[src,l,k] + s_tgt[tgt,l,k]) per bucketed edge (by-dst
 *     order).  Per head, the softmax over all edges entering a node (dpu_utils unsorted_segment_log_softmax
 *     + exp, rgat.py:147-151) is: m = segment max, p = exp(score - m[tgt]), den = segment sum of p,
 *     a = p / den[tgt] - the two segment reductions are tfgnn_graph_gather_reduce over view BY_DST_NODE with
 *     the identity as column array (so hub nodes use the long-row plan), the edge-parallel steps are
 *     tfgnn_rgat_edge_node_op.  The weighted sum out[v,k,:] = sum_e a_ek Y[(src,l),k,:] (rgat.py:154-163) is
 *     tfgnn_graph_gather_reduce(view BY_DST_NODE, ew_heads = K).
 * ------------------------------------------------------------------------------------------ */
int tfgnn_rgat_node_scores(const float* d_Y, const float* d_alpha, int64_t num_nodes, int num_edge_types,
                           int num_heads, int hidden_dim, float* d_s_src, float* d_s_tgt, void* stream);
int tfgnn_rgat_edge_scores(const int32_t* d_coll_by_dst, const int32_t* d_target_by_dst, const float* d_s_src,
                           const float* d_s_tgt, int64_t num_edges, int num_edge_types, int num_heads,
                           float* d_scores, void* stream);
/* mode 0: out[e,k] = exp(x[e,k] - node[tgt_e,k]);  mode 1: out[e,k] = x[e,k] / node[tgt_e,k] */
int tfgnn_rgat_edge_node_op(const float* d_x, const int32_t* d_target_by_dst, const float* d_node,
                            int64_t num_edges, int num_heads, int mode, float* d_out, void* stream);
/* backward pieces (tf.GradientTape in the reference):
 *   tfgnn_rgat_edge_dot:              da[e,k] = < d_agg[tgt_e,k,:], Y[(src_e,l_e),k,:] >
 *   tfgnn_rgat_edge_softmax_backward: dz[e,k] = a_ek (da_ek - t[tgt_e,k]) * leaky_relu'(z_ek),
 *                                     t[v,k] = sum over in-edges of a*da (a generic gather)
 *   tfgnn_rgat_scores_backward:       dY[(v,l),k,:] += ds_src[(v,l),k] alpha[l,k,:H/K] + ds_tgt[(v,l),k] alpha[l,k,H/K:] */
int tfgnn_rgat_edge_dot(const int32_t* d_coll_by_dst, const int32_t* d_target_by_dst, const float* d_Y,
                        const float* d_dagg, int64_t num_edges, int num_heads, int hidden_dim, float* d_da,
                        void* stream);
int tfgnn_rgat_edge_softmax_backward(const int32_t* d_coll_by_dst, const int32_t* d_target_by_dst,
                                     const float* d_s_src, const float* d_s_tgt, const float* d_att,
                                     const float* d_da, const float* d_t, int64_t num_edges, int num_edge_types,
                                     int num_heads, float* d_dz, void* stream);
int tfgnn_rgat_scores_backward(const float* d_ds_src, const float* d_ds_tgt, const float* d_alpha,
                               int64_t num_nodes, int num_edge_types, int num_heads, int hidden_dim,
                               float* d_dY, void* stream);
/* As above, the result dY' = dY + (score terms) written as an SP16 split operand (rows = nodes, L * H columns, one scale per
 * row) - the operand of dX = dY' W^T (tfgnn_sp_gemm_nt) in mode f16x2 - and, when update_fp32 != 0, back into d_dY as well
 * (the weight gradient X^T dY' stays on tfgnn_gemm: the rows of dY' carry attention weights and spread over more than the
 * 2^20 tfgnn_sp_gemm_tn's guard allows).  (H / K) % 4 == 0, L * H <= 2048 and a multiple of 16 (TFGNN_ERR_UNSUPPORTED otherwise). */
int tfgnn_rgat_scores_backward_sp(const float* d_ds_src, const float* d_ds_tgt, const float* d_alpha, float* d_dY,
                                  int update_fp32, int64_t num_nodes, int num_edge_types, int num_heads, int hidden_dim,
                                  void* d_dY_sp, float* d_inv_scale, void* stream);

/* Round 3: the per-target softmax of rgat.py:142-151 row by row over the node view (all incoming edges of a node, every
 * type) instead of edge scores + segment max + exp + segment sum + divide, and its gradient likewise:
 *   forward:  att[e, k] = softmax over the in-edges e of v of leaky_relu(s_src[(src_e, l_e), k] + s_tgt[(v, l_e), k])   [E, K], by-dst order;
 *             d_att_by_src (nullable): the same weights in the by-source edge order (for the backward pass's weighted gather)
 *   backward: dz[e, k]  = att (da - sum_{e' into v} att da) leaky_relu'(z)                  (the gradient w.r.t. the logits)
 * 1 <= num_heads <= 64 (TFGNN_ERR_UNSUPPORTED otherwise); a head count that is not a power of two runs on the lane layout
 * of the next power of two with the surplus lanes idle (3 heads: a quarter of them).  The arrays keep their stride num_heads.
 * Short rows take one wave, single-item rows of the long-row plan one workgroup, hub rows one workgroup PER ITEM with an
 * in-order combine of the items' (max, sum) pairs in between (d_workspace: tfgnn_rgat_attention_workspace_bytes); online
 * softmax, fixed reduction trees and orders: deterministic. */
size_t tfgnn_rgat_attention_workspace_bytes(const tfgnn_graph* graph, int num_heads);
int tfgnn_rgat_attention_forward(const tfgnn_graph* graph, const float* d_s_src, const float* d_s_tgt, int num_heads,
                                 float* d_att, float* d_att_by_src, void* d_workspace, size_t workspace_bytes, void* stream);
int tfgnn_rgat_attention_backward(const tfgnn_graph* graph, const float* d_s_src, const float* d_s_tgt, const float* d_att,
                                  const float* d_da, int num_heads, float* d_dz, void* d_workspace, size_t workspace_bytes,
                                  void* stream);
/* d alpha_l[k, :H/K] = sum_v ds_src[(v,l), k] Y[(v,l), k, :],  d alpha_l[k, H/K:] = sum_v ds_tgt[(v,l), k] Y[(v,l), k, :]
 * (gradient of the einsum of rgat.py:115-121 w.r.t. the attention parameters): d_alpha_grad [L, K, 2 H/K]; two-stage
 * reduction in a fixed order (workspace: tfgnn_rgat_alpha_grad_workspace_bytes). */
size_t tfgnn_rgat_alpha_grad_workspace_bytes(int64_t num_nodes, int num_edge_types, int hidden_dim);
int tfgnn_rgat_alpha_grad(const float* d_ds_src, const float* d_ds_tgt, const float* d_Y, int64_t num_nodes, int num_edge_types,
                          int num_heads, int hidden_dim, float* d_alpha_grad, void* d_workspace, size_t workspace_bytes,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Node -> graph pooling (layers/nodes_to_graph_representation.py:170-229).  node_to_graph_map is
 * sorted (data/graph_dataset.py:211-217), so segments are ranges ptr[g]..ptr[g+1].
 *   tfgnn_segment_offsets: ids [V] -> ptr [G+1]; synchronises once to report unsorted /
 *       out-of-range ids (tf.math.segment_sum raises InvalidArgument for both).
 *   tfgnn_segment_softmax: per (graph, head) dpu_utils unsorted_segment_softmax of the node scores
 *       (:178-186): exp(s - max) / (sum + 1e-7).  scores/out: [V, heads] with row strides ld.
 *   tfgnn_segment_weighted_sum: out[g,h,:] = sum_{v in g} w[v,h] * R[v,h,:] (:219-227); w NULL =
 *       tf.math.segment_sum (:204-210); mean=1 = tf.math.segment_mean (:211-217).
 *   *_backward: gradients of the two ops above (tf.GradientTape in the reference).
 * ------------------------------------------------------------------------------------------ */
int tfgnn_segment_offsets(const int32_t* d_ids, int64_t V, int64_t G, int32_t* d_ptr, void* stream);
/* The same without the validity read-back: no allocation, no synchronisation.  *d_error_flag (zeroed by the caller) gets
 * bit 0 = an id outside [0, G), bit 1 = ids not sorted; the caller reads it when it wants to know (the host mirror does so
 * once per batch and shares the offsets between the pooling layers, the global exchanges and the task head). */
int tfgnn_segment_offsets_async(const int32_t* d_ids, int64_t V, int64_t G, int32_t* d_ptr, int32_t* d_error_flag,
                                void* stream);
int tfgnn_segment_softmax(const float* d_scores, int64_t ld, int heads, const int32_t* d_ptr, int64_t G,
                          float* d_out, int64_t ld_out, void* stream);
int tfgnn_segment_weighted_sum(const float* d_R, const float* d_w, const int32_t* d_ptr, int64_t G, int GD,
                               int heads, int mean, float* d_out, void* stream);
int tfgnn_segment_weighted_sum_backward(const float* d_dOut, const float* d_R, const float* d_w,
                                        const int32_t* d_ids, const int32_t* d_ptr, int64_t V, int GD,
                                        int heads, int mean, float* d_dR, float* d_dW, void* stream);
int tfgnn_segment_softmax_backward(const float* d_w, const float* d_dw, int heads, const int32_t* d_ptr,
                                   int64_t G, float* d_ds, void* stream);

/* Layer-input dropout of the GNN stack (gnn.py:285-288; [ext] tf.nn.dropout scales kept units by
 * 1/(1-rate)).  d_mask receives 0 or 1/(1-rate) per element; the gradient is tfgnn_mul(dy, mask).
 * The stream of random numbers is this library's own (counter-based: element i of a call is a pure function of (seed, i)),
 * not TensorFlow's.  d_mask may be NULL (not stored); d_y == NULL (then d_x is ignored) only (re)generates the mask of
 * (seed, rate) - what tfgnn_sp_gemm_nt_dropout applies in its epilogue.
 *
 * The dropout mask generator (all of it fixed: tests/dropout_reference.py reproduces every mask exactly, and every kernel that
 * draws one - this entry, tfgnn_dropout_forward_sp, the epilogues of tfgnn_sp_gemm_nt_dropout in forward and gradient products,
 * tfgnn_gru_gates_backward_sp_dropout - draws this one).  32-bit wrap-around arithmetic unless stated:
 *   s0, s1     the low and the high word of splitmix64's output for `seed` (z = seed + 0x9E3779B97F4A7C15;
 *              z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31, in 64 bits).
 *              seed 0: z = 0xE220A8397B1DCDAF.
 *   threshold  ceil((double)rate * 2^24) of the FLOAT32 rate: 0.1f -> 0x19999A, 0.5f -> 0x800000, rate 0 -> 0 (all kept)
 *   scale      1.f / (1.f - rate), both operations in float32: the value of a kept mask element
 *   epoch e    (the device word below; read once per kernel):  e != 0:  s0 ^= lowbias32(e * 0x9E3779B9 + 0x7F4A7C15),
 *              s1 += e * 0x85EBCA6B;  e = 0: nothing.  rate 0 never reads the epoch.
 *   word       ONE per aligned group of four elements, g = index / 4 (64 bits):
 *                  word(g) = lowbias32((uint32)g ^ s0 ^ h) ^ s1,   h = 0 while g < 2^32, else lowbias32((g >> 32) * 0x9E3779B9 + 1)
 *              (the high-word term: tensors of more than 2^34 elements);
 *              lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *   element    e = index % 4 takes the 24-bit number  u = rotl(word, 8 e) >> 8  and is KEPT iff u >= threshold: mask = scale,
 *              else mask = 0.  y = x * mask in float32 (a dropped inf or NaN is NaN, as in tf.nn.dropout).
 *   index      = row * cols + column of the LOGICAL tensor the call describes (flat entries: the element's position in the
 *              call; products: output row - the row d_row_map names, where one is given - times N plus column), never an
 *              address: views, leading dimensions and alignment do not enter.
 * Every element's number is uniform, so P(kept) = 1 - threshold / 2^24, within 2^-24 of 1 - rate, and E[mask] = 1 within
 * 2^-23 / (1 - rate).  The four elements of a group are NOT independent: element e decides on a byte of its own (the top byte
 * of u, byte 3 - e of the word), but when that byte equals the threshold's top byte (probability 2^-8) the decision falls to
 * the two bytes below it, which are the deciding bytes of elements e + 1 and e + 2 (mod 4).  The correlation of two elements
 * of a group is at most 2^-8 plus terms of order 2^-16 / (rate (1 - rate)) (tests/test_dropout_reference_host.py derives and
 * enumerates it); it is 0 at rates whose threshold has sixteen zero low bits (0.5, 0.25, 0.125).  Elements of different
 * groups, seeds or epochs share no hash input.
 * seed 2^64 - 1 is RESERVED at the NT product entries (tfgnn_sp_gemm_nt_dropout and the entries built on it), where it selects
 * the mask-from-saved form; this entry, tfgnn_dropout_forward_sp and tfgnn_gru_gates_backward_sp_dropout take it as a seed. */
int tfgnn_dropout_forward(const float* d_x, float* d_y, float* d_mask, int64_t n, float rate,
                          uint64_t seed, void* stream);
/* The same dropout (same random numbers: element (r, c) draws that of flat index r * cols + c) that also writes its result
 * in the SP16 operand format with one power-of-two scale per row (see "Split fp16 operands"): the layer input is an
 * operand of the weight-gradient product downstream, and splitting it where it is produced saves one pass over it.
 * cols % 16 == 0, cols <= 512; d_out_sp 64-byte aligned rows of ld_out_sp_bytes >= 4 * cols; d_inv_scale [rows]. */
int tfgnn_dropout_forward_sp(const float* d_x, float* d_y, float* d_mask, int64_t rows, int64_t cols, float rate,
                             uint64_t seed, void* d_out_sp, int64_t ld_out_sp_bytes, float* d_inv_scale, void* stream);
/* The dropout EPOCH (round 5).  Every mask this library draws - tfgnn_dropout_forward / _sp, the epilogues of
 * tfgnn_sp_gemm_nt_dropout, the recomputed mask of tfgnn_gru_gates_backward_sp_dropout - is a function of (seed, element,
 * epoch), the epoch being one word of DEVICE memory the kernels read when they start.  It exists for steps replayed from a
 * captured hipGraph (tf2_gnn_amd.capture.CapturedStep): a replay re-launches the same kernels with the same seeds, so the
 * first node of the captured step is tfgnn_dropout_epoch_advance (a one-thread kernel: epoch += 1) and every replay draws
 * fresh masks, forward and backward kernels of one replay the same ones.  Epoch 0 - the state of a process that never
 * advances it - gives exactly the masks of (seed, element) alone.  _set stores a value (a kernel on `stream`), _get reads it
 * back (synchronises `stream`).  [ext] tf.nn.dropout draws new random numbers per call: gnn.py:285-288. */
int tfgnn_dropout_epoch_advance(void* stream);
int tfgnn_dropout_epoch_set(uint32_t value, void* stream);
int tfgnn_dropout_epoch_get(uint32_t* h_value, void* stream);
int tfgnn_mul(const float* d_a, const float* d_b, float* d_out, int64_t n, void* stream);

/* Inter-layer LayerNormalization of the GNN stack (gnn.py:157-161,318-321; [ext] Keras defaults
 * axis=-1, epsilon=1e-3).  backward: d_dx, and d_dy_xhat = dy * xhat whose column sum is d gamma
 * (d beta = column sum of dy; both via tfgnn_colsum). */
int tfgnn_layernorm_forward(const float* d_x, const float* d_gamma, const float* d_beta, float eps,
                            int64_t rows, int H, float* d_y, float* d_mean, float* d_rstd, void* stream);
int tfgnn_layernorm_backward(const float* d_dy, const float* d_x, const float* d_gamma, const float* d_mean,
                             const float* d_rstd, int64_t rows, int H, float* d_dx, float* d_dy_xhat,
                             void* stream);

/* dst[b, a, :] = src[a, b, :]: re-pack the stacked per-edge-type kernels [L, D, H] <-> [D, L, H]
 * (one bias-free kernel per edge type, gnn_edge_mlp.py:73-81) so that a layer's backward pass is two
 * large GEMMs. */
int tfgnn_permute_021(const float* d_src, int64_t A, int64_t B, int64_t C, float* d_dst, void* stream);
/* ------------------------------------------------------------------------------------------
 * Split-operand Dense products on the fp16 matrix cores ("f16x2", csrc/gemm_sp.hip): the same Keras Dense /
 * MatMul-gradient call sites as tfgnn_gemm (gnn_edge_mlp.py:100, rgcn.py:52-56, gnn.py:279,324-327,
 * models/graph_task_model.py:347-357), fp32 in / fp32 accumulate / fp32 out, with the operands handed over
 * already split so that the product kernel only moves data (LDS-DMA) and multiplies.
 *
 * SP16 operand format of an fp32 matrix [rows, cols] (cols % 16 == 0; the same number of bytes as the matrix):
 *   element (r, c) = h + l,  h, l fp16:  byte r * ld_bytes + (c / 16) * 64 + plane * 32 + (c % 16) * 2
 *   (plane 0 = h = fp16(x * 2^e), plane 1 = l = fp16(x * 2^e - h)), one power-of-two scale 2^e per row and per
 *   block of `scale_block` columns chosen so that the block maximum lies in [2^14, 2^15);
 *   d_inv_scale[r * (cols / scale_block) + b] = 2^-e.  |x - (h + l) 2^-e| <= 2^-22 |x| (elements within 2^-3 of the
 *   block maximum) or 2^-39 of the block maximum.
 * tfgnn_sp_split_rows: source element (r, c) = d_src[r * ld + (c / seg_len) * seg_stride + c % seg_len]
 *   (seg_len <= 0: plain row-major rows).  d_fixed_inv_scale (nullable, 1 float on the device): use this 2^-e for the
 *   whole tensor instead of per-block maxima (a caller-side bound; what the weight-gradient product needs).
 * tfgnn_sp_split_cols: SP16 row n, column k = d_src[k * ld + n] (a Keras kernel [K, N] -> the [N, K] operand).
 * tfgnn_sp_gemm_nt:   C[M,N] = epilogue( A[M,K] . B[N,K]^T ), A and B in SP16 (K contiguous);
 *   epilogue = act(. + bias) (+ C if accumulate), then * d_mul * act'(d_saved) as in tfgnn_gemm_grad_epilogue.
 *   a_scale_block: columns per scale block of A (0: K, i.e. one scale per row; < 0: d_a_inv_scale points to ONE scale
 *   for the whole tensor); B has one scale per row (d_b_inv_scale [N]); NULL scales = 1.  N % 128 == 0 (tiles of 320, 256 or 128 columns), K % 16 == 0; TFGNN_ERR_UNSUPPORTED otherwise.
 * ------------------------------------------------------------------------------------------ */
size_t tfgnn_sp_bytes(int64_t rows, int64_t cols);
int tfgnn_sp_split_rows(const float* d_src, int64_t ld, int64_t seg_len, int64_t seg_stride, int64_t rows, int64_t cols,
                        int scale_block, void* d_sp, int64_t ld_sp_bytes, float* d_inv_scale,
                        const float* d_fixed_inv_scale, void* stream);
int tfgnn_sp_split_cols(const float* d_src, int64_t ld, int64_t K, int64_t N, void* d_sp, int64_t ld_sp_bytes,
                        float* d_inv_scale, void* stream);
int tfgnn_sp_gemm_nt(int64_t M, int64_t N, int64_t K, const void* d_A_sp, int64_t lda_bytes, const float* d_a_inv_scale,
                     int a_scale_block, const void* d_B_sp, int64_t ldb_bytes, const float* d_b_inv_scale, float* d_C,
                     int64_t ldc, const float* d_bias, int act, int accumulate, const float* d_mul, int64_t ld_mul,
                     int act_of_saved, const float* d_saved, int64_t ld_saved, void* stream);
/* The same product whose epilogue ALSO writes the result as an SP16 operand with one power-of-two scale per row
 * (d_out_sp rows of ld_out_sp_bytes >= 4 N, 64-byte aligned; d_out_inv_scale [M]) - the operand of the next product
 * (a Dense layer behind a message-passing layer, the weight-gradient products of the backward pass) without a split
 * pass.  The row maximum is taken over the FINAL values (after bias / activation / the gradient factors), per COLUMN TILE
 * of the product (N = 128, 256 or 320: one scale per row; since round 5 also several tiles - N = 512 = 2 x 256, 640 = 2 x 320:
 * d_out_inv_scale [M][N / tile], an operand with scale blocks of one tile, a_scale_block of the next product); no
 * accumulation; d_C may be NULL when only the split form is needed. */
int tfgnn_sp_gemm_nt_sp(int64_t M, int64_t N, int64_t K, const void* d_A_sp, int64_t lda_bytes, const float* d_a_inv_scale,
                        int a_scale_block, const void* d_B_sp, int64_t ldb_bytes, const float* d_b_inv_scale, float* d_C,
                        int64_t ldc, const float* d_bias, int act, const float* d_mul, int64_t ld_mul, int act_of_saved,
                        const float* d_saved, int64_t ld_saved, void* d_out_sp, int64_t ld_out_sp_bytes,
                        float* d_out_inv_scale, void* stream);
/* tfgnn_sp_gemm_nt_dropout with the rows of A read through an index (round 5): product row r multiplies operand row
 * d_a_rows[r] (int32 [M], every entry in [0, M); NULL: row r) and takes that row's scales; the operand must be below 4 GB.
 * The input-gradient product dX = [G_0|..|G_{L-1}] W^T of the aggregate-first layers walks the by-source sums in the order of
 * their emptiness patterns this way (d_a_rows = d_row_map = TFGNN_G_PATTERN_NODE_BY_SRC, d_tile_kmask =
 * TFGNN_G_PATTERN_TILEMASK_BY_SRC) and skips the all-zero type blocks of a row tile, while the sums themselves stay in node
 * order, as the weight-gradient product needs them.  Skipped products are exact zeros: bit-equal to the unindexed call. */
int tfgnn_sp_gemm_nt_rows(int64_t M, int64_t N, int64_t K, const void* d_A_sp, int64_t lda_bytes, const float* d_a_inv_scale,
                          int a_scale_block, const int32_t* d_a_rows, const void* d_B_sp, int64_t ldb_bytes, const float* d_b_inv_scale,
                          float* d_C, int64_t ldc, const float* d_bias, int act, int accumulate, const float* d_mul, int64_t ld_mul,
                          int act_of_saved, const float* d_saved, int64_t ld_saved, float saved_scale, void* d_out_sp,
                          int64_t ld_out_sp_bytes, float* d_out_inv_scale, float dropout_rate, uint64_t dropout_seed,
                          const uint8_t* d_tile_kmask, const int32_t* d_row_map, void* stream);

/* Grouped rows (round 5; BASELINE configs[4]: the per-relation MLPs of RGIN / GNN_Edge_MLP over the non-empty (source, type)
 * rows, rgin.py:77-106, gnn_edge_mlp.py:84-107): the M product rows fall into num_groups consecutive groups, group g multiplies
 * ITS OWN [N, K] weight operand: group g's starts b_group_stride_bytes behind group g-1's, its column scales / bias
 * b_scale_group_stride elements behind (stacked operands: N * ldb_bytes and N; column blocks of ONE operand [N, G * K] - what
 * tfgnn_sp_split_cols makes of G stacked Keras kernels [G * K, N], one scale per row shared by the groups: 4 * K and 0).
 * d_tile_table: int32 [num_tiles][4] = {first row, rows (1..128), group, 0} - every row tile lies inside one group (the host
 * cuts each group into tiles of 128 rows; a binder builds it from the group offsets).  d_a_rows / a_src_rows as in
 * tfgnn_sp_gemm_nt_rows, with the source operand having a_src_rows rows (the first MLP layer reads the node states through the
 * row -> node index: no expanded copy of them is made).  The split-form result (d_out_sp) carries one scale per row and column
 * tile: N = 512 gives scale blocks of 256 columns - what the next grouped product takes as a_scale_block = 256.
 * 3 piece products per fp32 product where the bf16x3 grouped kernels (tfgnn_gemm_grouped_rows) spend 6. */
int tfgnn_sp_gemm_nt_grouped(int64_t M, int64_t N, int64_t K, const void* d_A_sp, int64_t lda_bytes, const float* d_a_inv_scale,
                             int a_scale_block, const int32_t* d_a_rows, int64_t a_src_rows, const int32_t* d_tile_table,
                             int64_t num_tiles, int num_groups, const void* d_B_sp, int64_t ldb_bytes, int64_t b_group_stride_bytes,
                             const float* d_b_inv_scale, int64_t b_scale_group_stride, float* d_C, int64_t ldc, const float* d_bias,
                             int act, const float* d_mul, int64_t ld_mul, int act_of_saved, const float* d_saved, int64_t ld_saved,
                             void* d_out_sp, int64_t ld_out_sp_bytes, float* d_out_inv_scale, void* stream);
/* dst row r = src row d_index[r] of an SP16 operand, with its scales_per_row scales (an index outside [0, src_rows) gives a
 * zero row).  The expanded operand of the grouped weight-gradient products: the K dimension of tfgnn_sp_gemm_tn cannot be
 * read through an index. */
int tfgnn_sp_gather_rows(const void* d_src_sp, int64_t ld_src_bytes, const float* d_src_inv_scale, int scales_per_row,
                         const int32_t* d_index, int64_t rows, int64_t src_rows, int64_t cols, void* d_dst_sp, int64_t ld_dst_bytes,
                         float* d_dst_inv_scale, void* stream);

/* tfgnn_sp_gemm_tn with a WIDER operand range (round 5): both operands' fragments carry per-k factors instead of one combined
 * factor on A.  Round 6: the two factors of row k share the deficit of the PAIR - (inv_a[k] / its maximum over the K range) x
 * (inv_b[k] / its maximum) = 2^-e is applied as 2^-ceil(e / 2) on A and 2^-floor(e / 2) on B (per scale block of A: the block
 * with the smallest deficit sets B's share) - so a row pair keeps >= 16 bits while its scale PRODUCT lies within 2^44 of the
 * largest of its K range (ranges of <= 2016 rows, factors computed in the kernel), whichever operand the spread comes from;
 * the spread flag is set beyond that (for pairs of non-zero rows).  For products whose rows are un-normalised sums on both sides (the
 * per-relation weight gradients of RGIN at arxiv scale: row scales over 2^19 and 2^21, their products over 2^25 - the combined
 * factor of tfgnn_sp_gemm_tn trips its 2^20 guard there).  Costs 2 (N / 32) packed multiplies more per k16 step (~+25 %) and
 * more K ranges (workspace: tfgnn_sp_gemm_tn_wide_workspace_bytes).  d_b_inv_scale is required.  Same result layout
 * arguments. */
size_t tfgnn_sp_gemm_tn_wide_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t a_total_cols, int a_scale_block);
int tfgnn_sp_gemm_tn_wide(int64_t M, int64_t N, int64_t K, const void* d_A_sp, int64_t lda_bytes, int64_t a_first_col,
                          const float* d_a_inv_scale, int64_t a_total_cols, int a_scale_block, const void* d_B_sp,
                          int64_t ldb_bytes, int64_t b_first_col, const float* d_b_inv_scale, float* d_C, int64_t group_rows,
                          int64_t stride_group, int64_t stride_row, int64_t stride_col, int accumulate, void* d_workspace,
                          size_t workspace_bytes, void* stream);

/* The wide-range product over ROW GROUPS of the same two operands in one launch (round 5; the kernel gradients dW_g = A_g^T B_g
 * of the per-relation MLPs): d_split_table int32 [num_splits][2] = (first row, rows <= 2016) of every K range, ranges of a group
 * consecutive; d_group_split_offsets int32 [num_groups + 1] = first range of every group.  Output g at d_C + g *
 * c_group_stride, element (m, n) at m * stride_row + n * stride_col.  Workspace: 4 * 512 * (a_total_cols / a_scale_block)
 * rounded up to 256, + num_splits * roundup(M, 128) * N * 4 bytes.  num_splits <= 512.
 * tfgnn_sp_gemm_tn_grouped_workspace_bytes returns that size - plus the tail of the trip words (2304 bytes) while the in-stream
 * repair is armed (tfgnn_sp_guard_repair below); 0 for a shape the product rejects.  A call whose workspace is smaller fails. */
size_t tfgnn_sp_gemm_tn_grouped_workspace_bytes(int64_t M, int64_t N, int64_t a_total_cols, int a_scale_block, int num_splits);
int tfgnn_sp_gemm_tn_grouped(int64_t M, int64_t N, const void* d_A_sp, int64_t lda_bytes, const float* d_a_inv_scale,
                             int64_t a_total_cols, int a_scale_block, const void* d_B_sp, int64_t ldb_bytes, const float* d_b_inv_scale,
                             int num_groups, const int32_t* d_group_split_offsets, int num_splits, const int32_t* d_split_table,
                             float* d_C, int64_t c_group_stride, int64_t stride_row, int64_t stride_col, void* d_workspace,
                             size_t workspace_bytes, void* stream);

/* K split INSIDE the launch of the NT product, for few row tiles (round 5; BASELINE configs[0]: a PPI batch of 7 110 nodes is 56
 * row tiles - 56 workgroups each streaming the whole weight operand while 200 CUs idle, and the product takes as long as at
 * 30 000 nodes).  With a workspace registered here, products of at most 112 output tiles and K >= 480 launch S = 2..4
 * workgroups per tile (S * tiles <= 232: all resident at once); splits 1 .. S-1 hand their raw accumulators to split 0
 * through the workspace (write-through stores + one flag word each), split 0 adds them in split order - the result is
 * bit-reproducible, though not bit-equal to the unsplit product's (another summation order; same error class) - and runs
 * the epilogue.  No extra launch, no extra pass.  Layout: [64 KB of flags][slabs of 128 x tile-width floats]; 32 MB cover
 * every shape eligible for the K split.  The
 * library keeps the flags zero between launches (each reducer clears what it consumed), which is what makes a product
 * captured in a hipGraph replayable.  ONE workspace per process, owned by the device that was current at registration
 * (round 6): a product on another device is never split; a split product on another STREAM than the previous one
 * first waits (host side) for that stream, so two split products never share the flags in flight (a stream under capture
 * cannot wait: synchronise the device before capturing, as capture.CapturedStep does; while another stream is capturing split
 * products, a product stays unsplit).  d_workspace NULL / too small: no split (the default).  The call waits for the device.
 * A reducer that gives up waiting for a producer (~1 s; never expected) leaves ITS product incomplete: the next product call
 * then fails with TFGNN_ERR_HIP and a message, after clearing the flags (a late producer may have left one set).
 * _status: enable >= 0 switches the split on / off (the workspace stays); *timed_out (may be NULL) = number of such timeouts
 * so far; *split_launches (may be NULL) = products launched with a split so far (tests assert that the path under test
 * really ran); returns 1 if splits can happen. */
int tfgnn_sp_gemm_nt_set_splitk_workspace(void* d_workspace, size_t bytes);
int tfgnn_sp_gemm_nt_splitk_status(int enable, int* timed_out, int64_t* split_launches);

/* The superset: tfgnn_sp_gemm_nt / _sp (d_out_sp may be NULL) with the layer-input dropout of the NEXT op in the epilogue
 * (gnn.py:285-288 - the producer of a layer's input drops it, so the stand-alone pass over [V, H], its mask tensor and the
 * split pass disappear): the result, after bias / activation / the gradient factors, is multiplied by the mask
 * tfgnn_dropout_forward draws for (dropout_seed, dropout_rate) at element index row * N + column (rate 0: no dropout).
 * In a gradient product the same argument RECOMPUTES the forward mask (no mask tensor is read), and `saved_scale` lets
 * d_saved be the DROPPED activation: the derivative is taken at d_saved * saved_scale (= 1 - rate: the kept values carry
 * 1 / (1 - rate); dropped positions have mask 0 anyway).  dropout_seed = UINT64_MAX in a gradient product whose saved tensor
 * is a dropped RELU output: no mask is computed at all - that tensor is positive exactly where the unit was kept and active,
 * relu'(d_saved) carries the mask's zeros and the epilogue only applies 1 / (1 - rate).
 * d_tile_kmask (uint8 per 128-row tile of A, NULL = all) with a_scale_block > 0: bit b of a tile's byte says whether scale block b
 * of K holds anything but zeros in that tile - the product skips the other blocks (at most 8 blocks; TFGNN_G_PATTERN_TILEMASK_BY_DST
 * for an operand written through TFGNN_VIEW_BY_DST_TYPED_PATTERN).  d_row_map (int32 [M], NULL = identity): row r of the product is
 * written (and its d_mul / d_saved / dropout index taken) at row d_row_map[r] (TFGNN_G_PATTERN_NODE_BY_DST: back to node order). */
int tfgnn_sp_gemm_nt_dropout(int64_t M, int64_t N, int64_t K, const void* d_A_sp, int64_t lda_bytes, const float* d_a_inv_scale,
                             int a_scale_block, const void* d_B_sp, int64_t ldb_bytes, const float* d_b_inv_scale, float* d_C,
                             int64_t ldc, const float* d_bias, int act, int accumulate, const float* d_mul, int64_t ld_mul,
                             int act_of_saved, const float* d_saved, int64_t ld_saved, float saved_scale, void* d_out_sp,
                             int64_t ld_out_sp_bytes, float* d_out_inv_scale, float dropout_rate, uint64_t dropout_seed,
                             const uint8_t* d_tile_kmask, const int32_t* d_row_map, void* stream);

/* tfgnn_sp_gemm_tn: the weight-gradient product C[m, n] = sum_k A[k, a_first_col + m] B[k, b_first_col + n] of two SP16
 * operands stored with K as the row index (dW = X^T G of the Dense / edge-MLP kernels, tf.GradientTape in
 * models/graph_task_model.py:347-357).  Scales: A one 2^-e per (row, block of a_scale_block columns) at
 * d_a_inv_scale[k * (a_total_cols / a_scale_block) + b] (a_scale_block >= 32), B one per row (d_b_inv_scale[k]; NULL =
 * 1) - exactly what the producers write.  A per-row scale is a per-k factor of this product: a first pass turns the two
 * scale arrays into one fp16 factor <= 1 per (k, block) - the scale product over its maximum over k, a power of two - which
 * the kernel multiplies into the A fragments; a row whose scale product is 2^-j of the largest keeps 22 bits while
 * j <= 13, 35 - j bits after that, and drops out beyond 2^-24.
 * M % 16 == 0 (row tiles are 128 columns of A; the last one may run past M: it reads neighbouring bytes of the operand rows and
 * its surplus result rows stay in the workspace), N % 128 == 0, first columns multiples of 16.  Split-K with a deterministic second pass that also
 * scatters the result:
 *   C[(m / group_rows) * stride_group + (m % group_rows) * stride_row + n * stride_col] (+)= value
 * (row-major [M, N]: group_rows = M, stride_row = N, stride_col = 1; dW of stacked kernels [L, D, H] from m = (l, h),
 * n = d: group_rows = H, stride_group = D * H, stride_row = 1, stride_col = H).  d_workspace: 256-byte aligned,
 * tfgnn_sp_gemm_tn_workspace_bytes bytes. */
/* ---- small passes that share a launch ------------------------------------------------------------------------------
 * Around the big kernels of a layer sit passes of 5-15 us each that are bound by launch and dependent-load latency, not by
 * work: weight matrices into SP16 form, the column maxima of a long one.  A `tfgnn_aux_job` describes one of
 * them; tfgnn_aux_launch runs up to 8 per launch (more: several launches), every job on its own workgroups - the launch
 * takes as long as its longest job.  Jobs of one call must be independent of each other.  The *_job / *_jobs functions FILL a
 * job (host memory, nothing is launched for it) with exactly the work the function of the same name without the suffix would
 * have launched; a job holds device pointers - keep the buffers alive until the launch has been issued.  The caller that
 * fills jobs launches them itself, before the first kernel that reads their results: the library keeps no queue of them.  (No reference counterpart: TensorFlow schedules these ops one kernel each.) */
typedef struct tfgnn_aux_job {
  int kind;            /* 0: nothing to do */
  unsigned num_blocks; /* workgroups of 256 threads */
  unsigned char payload[248];
} tfgnn_aux_job;
int tfgnn_aux_launch(const tfgnn_aux_job* jobs, int num_jobs, void* stream);
int tfgnn_sp_split_rows_job(const float* d_src, int64_t ld, int64_t seg_len, int64_t seg_stride, int64_t rows, int64_t cols,
                            int scale_block, void* d_sp, int64_t ld_sp_bytes, float* d_inv_scale,
                            const float* d_fixed_inv_scale, tfgnn_aux_job* job);
int tfgnn_sp_split_cols_job(const float* d_src, int64_t ld, int64_t K, int64_t N, void* d_sp, int64_t ld_sp_bytes,
                            float* d_inv_scale, tfgnn_aux_job* job);
/* tfgnn_sp_split_cols for LONG K (round 6; the stacked kernels of many relations, BASELINE configs[4]: [40 * 512, 512]): the
 * one-pass job lets each of its K slices take the column maxima over all of K itself - 64-byte row pieces, the matrix read 8
 * times.  Two jobs instead: *maxima_job (whole rows, each byte once, per-slab maxima into d_colmax_workspace,
 * tfgnn_sp_split_cols_two_pass_bytes(K, N) bytes; 0 = K is short, the one-pass job is used and *maxima_job is empty) must run
 * in an EARLIER launch than *split_job.  Same operand, bit for bit (a maximum does not depend on the order). */
size_t tfgnn_sp_split_cols_two_pass_bytes(int64_t K, int64_t N);
int tfgnn_sp_split_cols_jobs(const float* d_src, int64_t ld, int64_t K, int64_t N, void* d_sp, int64_t ld_sp_bytes,
                             float* d_inv_scale, float* d_colmax_workspace, size_t workspace_bytes, tfgnn_aux_job* maxima_job,
                             tfgnn_aux_job* split_job);
/* tfgnn_graph_gather_reduce_sp.  *combine_job used to receive the combine pass of the long buckets; the gather now combines
 * them inside its own launch, so the job always comes back empty (kind 0).  Kept for C callers written against that form:
 * nothing in this package calls it any more (the Python wrappers and the layer-level entry points use the plain form). */
int tfgnn_graph_gather_reduce_sp_deferred(const tfgnn_graph* graph, int view, const int32_t* d_col_override,
                                          const float* d_edge_weight, const float* d_row_scale, const float* d_in,
                                          int64_t ld_in, int width, void* d_out_sp, int64_t ld_out_sp_bytes,
                                          float* d_inv_scale, const float* d_fixed_inv_scale, void* d_workspace,
                                          size_t workspace_bytes, tfgnn_aux_job* combine_job, void* stream);

size_t tfgnn_sp_gemm_tn_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t a_total_cols, int a_scale_block);
/* Guard of the limit above: the factor pass of every tfgnn_sp_gemm_tn sets a library-wide flag (host-visible without a
 * stream synchronisation; it trails the device by however far the stream is behind) when a NON-ZERO operand row lies more
 * than 2^20 below the largest row scale of its column block.  Between 2^-13 and 2^-20 a row keeps 35 - j bits relative to
 * itself and its ABSOLUTE error stays <= 2^-39 of the largest rows' elements - far below the fp32 rounding of the sum (the
 * measured error of the product against fp64, relative to sum |a||b|, as a function of the spread: tests/test_gpu_f16x2_mode.py,
 * profiles/parity_r03.json); beyond 2^-20 fewer than 15 bits are left and at 2^-24 the row drops out.  Returns the flag
 * (0 / 1), clears it when reset != 0.  The host mirror (tf2_gnn_amd.ops) routes the split-operand layer paths to the
 * exact bf16x3 kernels from the next call on once the flag is seen. */
int tfgnn_sp_spread_flag(int reset);
/* In-stream repair of a tripped product (opt-in; off unless the environment sets TFGNN_GUARD_REPAIR to a non-zero number).
 * While armed, every tfgnn_sp_gemm_tn / tfgnn_sp_gemm_tn_wide - also the one inside tfgnn_mp_backward - enqueues on the
 * caller's stream: a memset node that zeroes a trip word in a 256-byte tail of the call's own workspace (the two
 * *_workspace_bytes functions return 256 bytes more while armed, exactly the unarmed value otherwise), the unchanged product
 * kernels with their guard pointed at that word INSTEAD of the library-wide flag, a repair kernel, and the unchanged reduce
 * pass.  The repair kernel returns at once while the word is 0.  Otherwise it recomputes every split-K slab of the WHOLE
 * product in fp32 (FMA, ascending k: a fixed order) straight from the SP16 operands, element = (h + l) * inv_scale, skipping
 * (k, block) pairs with the all-zero marker scale as the product does, and sets the reference scales the reduce pass
 * multiplies back to 1 - the result lands through the same accumulate / scatter / column-range path as any other, and is
 * right in the very pass that tripped.  No host synchronisation and no allocation at launch time: the sequence can be captured
 * into a hipGraph and every replay repairs itself.  A covered product no longer raises tfgnn_sp_spread_flag, so nothing
 * demotes the mode.
 * tfgnn_sp_gemm_tn_grouped is covered too, range by range: its tail (tfgnn_sp_gemm_tn_grouped_workspace_bytes grows by it while
 * armed) holds one trip word per K range of the split table plus one "counted" word, all zeroed by one small kernel in front
 * of the product (a kernel node in a hipGraph, where the plain products have a 4-byte memset node); a range that sees a pair
 * beyond the guard sets its own word, and the repair kernel rewrites the slab of that range alone (same
 * arithmetic) and sets that range's reference scales to 1.  The other ranges of the group keep what the product wrote; the
 * grouped reduce pass multiplies every slab by its own reference and adds them in range order, so the result depends only on
 * the operands and the tables.  A grouped launch counts as ONE repaired product, however many of its ranges tripped.
 * tfgnn_sp_guard_repair: on = 1 arms, 0 disarms, -1 only queries; returns the previous state (0 / 1) or a negative error
 * code.  Arming allocates a device counter: not legal while a stream is capturing (arm before the capture).
 * tfgnn_sp_repair_stats: out2[0] = products enqueued with repair armed (host counter), out2[1] = products repaired (device
 * counter of the current device); reset != 0 clears both.  Waits for the device: not legal while a stream is capturing. */
int tfgnn_sp_guard_repair(int on);
int tfgnn_sp_repair_stats(int64_t* out2, int reset);
int tfgnn_sp_gemm_tn(int64_t M, int64_t N, int64_t K, const void* d_A_sp, int64_t lda_bytes, int64_t a_first_col,
                     const float* d_a_inv_scale, int64_t a_total_cols, int a_scale_block, const void* d_B_sp,
                     int64_t ldb_bytes, int64_t b_first_col, const float* d_b_inv_scale, float* d_C, int64_t group_rows,
                     int64_t stride_group, int64_t stride_row, int64_t stride_col, int accumulate, void* d_workspace,
                     size_t workspace_bytes, void* stream);
/* The reduce pass of a weight-gradient product carried by the NT product that follows it.  A weight gradient dW = X^T G and
 * the input gradient dX = G W^T of one layer are independent, and nothing on the critical path reads dW - so the reduce pass
 * (its own launch behind tfgnn_sp_gemm_tn: splits x M x N partial floats summed in split order) can run on the CUs the NT
 * product's row tiles leave free, as extra workgroups BEHIND the product's own in the same grid.
 *   tfgnn_sp_gemm_tn_product   tfgnn_sp_gemm_tn up to and including the product (and the armed repair pass); *job receives the
 *                               reduce pass instead of a launch.  Same operands, checks, workspace and arithmetic: dW comes out
 *                               bit for bit as tfgnn_sp_gemm_tn writes it.  A product whose reduction cannot be carried
 *                               runs it at once and hands back an empty job (num_blocks 0).
 *   tfgnn_sp_gemm_nt_rows_tail  tfgnn_sp_gemm_nt_rows whose launch carries *job (NULL or empty: exactly tfgnn_sp_gemm_nt_rows) on
 *                               job->num_blocks extra workgroups; they wait for nothing - stream order has finished the TN
 *                               product - so the call must be enqueued on the stream of, and after, the deferred product.
 *                               M = 0 (nothing to multiply) runs the job in a launch of its own.
 *   tfgnn_tn_reduce_launch      the job in a launch of its own (what tfgnn_sp_gemm_tn does); an empty job: nothing.
 * The caller that takes a job runs it exactly once, through one of the two, before anything reads dW or reuses the product's
 * workspace: a job holds device pointers into that workspace (partials, reference scales, trip words), which stays untouched
 * until the job has been issued.  It may NOT overlap the K-split workspace of the NT product
 * (tfgnn_sp_gemm_nt_set_splitk_workspace) - both are live in the carrying launch; an overlap is refused.  The library keeps
 * no queue of jobs.  num_blocks is filled from the size of the reduction (one workgroup per 512 elements, at most 1024);
 * a caller may change it (> 0).  tfgnn_tn_reduce_counts: out_counts[0] = reduce passes launched on their own so far (the plain
 * and the grouped), [1] = passes carried by an NT launch (host counters, like tfgnn_launch_counts - whose TFGNN_KFAM_SP_TN /
 * TFGNN_KFAM_SP_NT keep counting products and NT launches). */
typedef struct tfgnn_tn_reduce_job {
  unsigned num_blocks; /* 0: nothing to do */
  unsigned reserved;
  unsigned char payload[184];
} tfgnn_tn_reduce_job;
int tfgnn_sp_gemm_tn_product(int64_t M, int64_t N, int64_t K, const void* d_A_sp, int64_t lda_bytes, int64_t a_first_col,
                              const float* d_a_inv_scale, int64_t a_total_cols, int a_scale_block, const void* d_B_sp,
                              int64_t ldb_bytes, int64_t b_first_col, const float* d_b_inv_scale, float* d_C, int64_t group_rows,
                              int64_t stride_group, int64_t stride_row, int64_t stride_col, int accumulate, void* d_workspace,
                              size_t workspace_bytes, tfgnn_tn_reduce_job* job, void* stream);
int tfgnn_tn_reduce_launch(const tfgnn_tn_reduce_job* job, void* stream);
int tfgnn_tn_reduce_counts(int64_t* out_counts, int n);
int tfgnn_sp_gemm_nt_rows_tail(int64_t M, int64_t N, int64_t K, const void* d_A_sp, int64_t lda_bytes, const float* d_a_inv_scale,
                               int a_scale_block, const int32_t* d_a_rows, const void* d_B_sp, int64_t ldb_bytes,
                               const float* d_b_inv_scale, float* d_C, int64_t ldc, const float* d_bias, int act, int accumulate,
                               const float* d_mul, int64_t ld_mul, int act_of_saved, const float* d_saved, int64_t ld_saved,
                               float saved_scale, void* d_out_sp, int64_t ld_out_sp_bytes, float* d_out_inv_scale, float dropout_rate,
                               uint64_t dropout_seed, const uint8_t* d_tile_kmask, const int32_t* d_row_map,
                               const tfgnn_tn_reduce_job* job, void* stream);

/* Tensor-wide scales (d_fixed_inv_scale of the SP16 producers; tfgnn_sp_gemm_nt takes such an operand with a_scale_block < 0):
 * tfgnn_absmax gives *d_out = max(*d_out, scale * max |x|)
 * (start from 0; order-independent, so reproducible), tfgnn_sp_inv_scale_from_bound turns a bound into the 2^-e that
 * puts it in [2^14, 2^15).  A bound may exceed the true maximum (e.g. max |d_pre| times the largest weighted out-degree
 * for the gathered gradient): every factor of two costs one bit of the 18 the format has beyond fp32's significand. */
int tfgnn_absmax(const float* d_x, int64_t n, float scale, float* d_out, void* stream);
int tfgnn_sp_inv_scale_from_bound(const float* d_bound, float* d_inv_scale, void* stream);

/* tfgnn_graph_gather_reduce with per-head edge weights that ALSO writes, per edge e of the view and head k,
 *   d_dot_out[pos(e) * ew_heads + k] = sum_{f in head k} d_in[col(e), f] * d_dot_rows[r(e) * ld_dot + f]
 * r(e) = the row of the view that holds the edge, pos(e) = d_dot_pos[e] (NULL: the edge's position in the view's order).
 * Reference: the gradient of the attention-weighted message sum w.r.t. the attention values (what tf.GradientTape derives for
 * tf2_gnn/layers/message_passing/rgat.py:153-163) - on the by-source gather of the backward pass that reads d_agg[target(e)]
 * anyway, with d_dot_rows = Y and d_dot_pos = TFGNN_G_SRC2DST_POS.  tfgnn_graph_gather_dot_supported: 1 when the head width
 * (4 .. 64 floats, a power of two) fits the kernel's lane groups, else 0 (callers use tfgnn_rgat_edge_dot). */
int tfgnn_graph_gather_dot_supported(int width, int ew_heads);
int tfgnn_graph_gather_reduce_dot(const tfgnn_graph* g, int view, const float* d_edge_weight, int ew_heads, const float* d_in,
                                  int64_t ld_in, int width, float* d_out, int64_t ld_out, const float* d_dot_rows, int64_t ld_dot,
                                  const int32_t* d_dot_pos, float* d_dot_out, void* d_workspace, size_t workspace_bytes,
                                  void* stream);

/* tfgnn_graph_gather_reduce (plain sums: embedding_lookup + 1/(c+1e-7) scaling + unsorted_segment_sum,
 * message_passing.py:197-206,172-174, gnn_edge_mlp.py:102-106) writing its rows directly as the SP16 operand of
 * tfgnn_sp_gemm_* - the [V, L*D] matrix of per-(node, type) sums is never stored in fp32.  Row r of the view gets
 * its own scale d_inv_scale[r] (for a typed view the rows (v, l) are the (row v, scale block l) of the [V, L*width]
 * operand), or every row uses the caller's *d_fixed_inv_scale.  width % 16 == 0, width <= 512. */
int tfgnn_graph_gather_reduce_sp(const tfgnn_graph* graph, int view, const int32_t* d_col_override,
                                 const float* d_edge_weight, const float* d_row_scale, const float* d_in, int64_t ld_in,
                                 int width, void* d_out_sp, int64_t ld_out_sp_bytes, float* d_inv_scale,
                                 const float* d_fixed_inv_scale, void* d_workspace, size_t workspace_bytes, void* stream);
/* tfgnn_graph_gather_reduce_sp into an operand that ALREADY HOLDS the rows of the view's empty buckets.  Which buckets are
 * empty depends on the graph and the view, not on d_in: an operand that stays with the graph needs its zero rows and their
 * marker scales written once, not once per layer (RGCN H = 320 on 30 000 nodes: 45 % of the buckets, 69 MB per launch).
 * keep_empty_rows == 0: exactly tfgnn_graph_gather_reduce_sp.  keep_empty_rows != 0: the launch covers the non-empty buckets
 * only - an empty bucket's row of d_out_sp and its entry of d_inv_scale are neither read nor written; every other row comes out
 * bit for bit as above (same kernel, same order of the edges).
 * CONTRACT of keep_empty_rows != 0 - the caller promises, and the library cannot check without another pass over the operand:
 *   - d_out_sp / d_inv_scale were last written, in full, by a gather of the SAME graph handle, view, width and
 *     ld_out_sp_bytes that wrote every row (keep_empty_rows == 0, or a launch that fell back as described below);
 *   - that gather had the same d_row_scale VALUES (or NULL both times): an empty row holds 0 * row_scale, which is NaN where
 *     the scale is infinite or NaN, so a changed scale array needs a filling launch;
 *   - nothing else has written to either array since (gathers with keep_empty_rows != 0 in between are fine).
 * The request is honoured for the full-row views (0 - 3 and TFGNN_VIEW_BY_DST_TYPED_PATTERN) with per-row scales
 * (d_inv_scale); with d_fixed_inv_scale, on a compact view (which has no empty rows), on a handle whose view has no empty
 * bucket or no length-ordered row list, the launch is the filling one of tfgnn_graph_gather_reduce_sp. */
int tfgnn_graph_gather_reduce_sp_keep_empty(const tfgnn_graph* graph, int view, const int32_t* d_col_override,
                                            const float* d_edge_weight, const float* d_row_scale, const float* d_in,
                                            int64_t ld_in, int width, void* d_out_sp, int64_t ld_out_sp_bytes,
                                            float* d_inv_scale, const float* d_fixed_inv_scale, void* d_workspace,
                                            size_t workspace_bytes, int keep_empty_rows, void* stream);

/* [batch, rows, cols] -> [batch, cols, rows] (LDS-tiled).  Used to hand the GEMMs K-contiguous weights
 * (W^T of gnn_edge_mlp.py:100 / rgcn.py:52-56 kernels) and to bring dW^T = G^T X back to the [L, D, H] layout. */
int tfgnn_transpose_batched(const float* d_src, int64_t batch, int64_t rows, int64_t cols, float* d_dst,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * Task metrics behind the path: the losses the reference differentiates
 * and the per-batch numbers its epoch loop aggregates.  One streaming pass + a fixed-order two-stage
 * reduction (reproducible run to run); d_workspace: tfgnn_task_metrics_workspace_bytes() bytes.
 *   tfgnn_sigmoid_ce_metrics: NodeMulticlassTask._fast_task_metrics and micro_f1
 *       (models/node_multiclass_task.py:10-23,62-70).  logits / labels [V, C] fp32 (labels 0 / 1);
 *       d_metrics[0] = mean over nodes of the per-node sum of [ext] tf.nn.sigmoid_cross_entropy_with_logits,
 *       d_metrics[1] = micro-F1 of round(sigmoid(logits)) against int32(labels) (nan when undefined, as
 *       there); d_counts (optional) = {true pos, false pos, false neg}; d_dlogits (optional, [V, C]
 *       contiguous) = d loss / d logits = (sigmoid(x) - z) / V.
 *   tfgnn_regression_metrics: tf.losses.mean_squared_error / mean_absolute_error of per-graph outputs
 *       (models/graph_regression_task.py:157-158, models/qm9_regression.py:122-123): d_metrics = {mse, mae};
 *       d_dpred (optional) = d mse / d pred = 2 (pred - target) / G.
 *   tfgnn_binary_ce_metrics: GraphBinaryClassificationTask.compute_task_metrics
 *       (models/graph_binary_classification_task.py:31-58) from the per-graph LOGITS x and targets y (0 / 1), [G] fp32.
 *       p = sigmoid(x), pc = min(max(p, eps), hi) with eps = float32(1e-7), hi = float32(1) - eps;
 *       d_metrics[0] = mean over graphs of -(y log(pc + eps) + (1 - y) log(1 - pc + eps)): [ext]
 *       tf.keras.losses.binary_crossentropy(from_logits=False) as the Keras backend writes it for a probability
 *       input, PARITY UNPINNED (some TF versions, inside tf.function, recognise the Sigmoid producer and evaluate
 *       the logits form instead; the two differ only where p is clipped); d_metrics[1] = num_correct / G, where the
 *       prediction rint(p) (half to even: a logit of exactly 0 predicts 0, as tf.math.round) equals y;
 *       d_prob (optional, [G]) = p; d_counts (optional) = {true pos, false pos, true neg, false neg}, num_correct =
 *       tp + tn; d_dlogits (optional, [G]) = d loss / d logit =
 *       (-(y / (pc + eps)) + (1 - y) / (1 - pc + eps)) p (1 - p) / G where eps <= p <= hi and exactly 0 outside
 *       (the gradient of clip_by_value).
 * ------------------------------------------------------------------------------------------ */
size_t tfgnn_task_metrics_workspace_bytes(void);
int tfgnn_sigmoid_ce_metrics(const float* d_logits, int64_t ld_logits, const float* d_labels, int64_t ld_labels,
                             int64_t V, int64_t C, float* d_metrics, int64_t* d_counts, float* d_dlogits,
                             void* d_workspace, size_t workspace_bytes, void* stream);
int tfgnn_regression_metrics(const float* d_pred, const float* d_target, int64_t G, float* d_metrics,
                             float* d_dpred, void* d_workspace, size_t workspace_bytes, void* stream);
int tfgnn_binary_ce_metrics(const float* d_logits, const float* d_target, int64_t G, float* d_prob, float* d_metrics,
                            int64_t* d_counts, float* d_dlogits, void* d_workspace, size_t workspace_bytes,
                            void* stream);

/* tfgnn_softmax_ce_metrics: weighted softmax cross-entropy of per-node logits against ONE class per node, with its
 * accuracy counts, argmax and gradient (NodeClassificationTask; the reference has no counterpart, PARITY UNPINNED).
 * d_logits [V, C] fp32, row stride ld_logits >= C.  The class of node v is the fp32 d_labels[v * ld_labels], its weight
 * w_v the fp32 d_weights[v * ld_weights], or 1 when d_weights is NULL: element strides, so labels and weights may be two
 * columns of one [V, 2] array.  d_workspace: tfgnn_softmax_ce_workspace_bytes() bytes, 8-byte aligned.
 *   counted   node v is counted iff w_v > 0 and its label is an integer in [0, C).  A label of -1, one >= C, a fractional
 *             or NaN label, and a zero, negative or NaN weight all make the node uncounted: it adds nothing to any sum,
 *             its d_dlogits row is exactly 0, its d_pred is still written.
 *   W         sum of w_v over the counted nodes, added in double in a fixed order.
 *   loss      d_metrics[0] = sum over counted v of w_v (logsumexp(x_v) - x_v[y_v]) / W.  With m the row maximum and
 *             s = sum_c expf(x_v[c] - m) in fp32, the row's value is (double)m - (double)x_v[y_v] + (double)logf(s);
 *             rows are added in double.  W == 0 (no counted node): loss = 0 and every d_dlogits entry is 0.
 *   pred      d_pred[v] (optional, int32 [V]) = the lowest index of the row maximum (the tie rule of np.argmax); a NaN
 *             entry takes part as -inf.
 *   counts    d_counts (optional, int64 [2]) = {counted nodes with pred == label, counted nodes};
 *             d_metrics[1] = accuracy = correct / counted in double, 0 / 0 -> nan like the micro-F1.
 *   gradient  d_dlogits (optional, row stride ld_dlogits >= C; columns >= C are not touched):
 *             d_dlogits[v, c] = (w_v / W) (softmax(x_v)[c] - [c == y_v]) for counted v.
 *   NaN       a NaN logit in a counted row makes the loss NaN (and that row's gradient); it is not hidden.
 *   C == 1    is legal: loss 0, gradient 0, prediction 0.
 * Refused before any launch: V <= 0 or C <= 0 ("empty batch"), C > 2^24 (fp32 labels stop being exact), NULL d_logits /
 * d_labels / d_metrics, ld_logits < C, ld_dlogits < C, an element stride < 1, a short or misaligned workspace.
 * At most three launches, no allocation, no host synchronisation, capturable: (1) the weight pass reduces W and the number
 * of counted nodes over the V labels and weights (4 - 8 bytes per node against 8 C for the main pass), at most 64 partials;
 * (2) the main pass - every wave adds those partials up in the same fixed order, so the gradient is scaled by the same W
 * everywhere - leaves one partial per workgroup; (3) the fixed-order final stage.  d_metrics and d_counts are bit-identical
 * run to run and whether or not d_dlogits / d_pred are requested.
 * Row strategy of the main pass, by C: a row is shared by a group of G lanes, lane j of the group holding columns j, j + G,
 * ... in 8 registers, and a wave works on 64 / G consecutive rows at once: G = 4 for C <= 32, 8 for C <= 64, 16 for
 * C <= 128, 32 for C <= 256, 64 for C <= 512; every logit is read once and all reductions are cross-lane.  C > 512: one
 * wave per row, a running maximum and rescaled sum per lane merged across the wave, and a second read of the row for the
 * gradient.  The switches are at C = 32, 64, 128, 256 and 512. */
size_t tfgnn_softmax_ce_workspace_bytes(void);
int tfgnn_softmax_ce_metrics(const float* d_logits, int64_t ld_logits, const float* d_labels, int64_t ld_labels,
                             const float* d_weights, int64_t ld_weights, int64_t V, int64_t C, float* d_metrics,
                             int64_t* d_counts, float* d_dlogits, int64_t ld_dlogits, int32_t* d_pred,
                             void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Link prediction with a DistMult decoder (LinkPredictionTask, csrc/link.hip; the reference has no counterpart, PARITY
 * UNPINNED).  A triple e = (u_e, t_e, v_e) is a typed edge: source node, relation, target node.  Common to the three calls:
 * d_H [V, D] fp32 node representations, row stride ld_H >= D; d_R [T, D] fp32 relation embeddings, contiguous;
 * triples / queries int32 [N, 3] rows (u, t, v), contiguous.  1 <= D <= 1024, 1 <= V, T < 2^31, 1 <= N <= 2^30.  Every index
 * must be in range (0 <= u, v < V, 0 <= t < T) and every table well formed: the kernels do NOT check that, the host side that
 * builds the arrays does (tf2_gnn_amd/ops.py build_triple_tables validates).  No call allocates or synchronises with the host;
 * all are capturable on the one stream they are given.  No floating-point atomic is used: every floating-point sum below has
 * an order that is a function of the arguments and tables only - not of timing, and not of which optional outputs are
 * requested.  Bad arguments are refused before any launch.
 *   score     s_e = sum_d H[u, d] R[t, d] H[v, d] in fp32, by ONE device routine shared by every kernel of the three calls:
 *             lane l of a wave adds the columns d = l, l + 64, l + 128, ... in ascending order as
 *             p = fma(H[u, d] * R[t, d], H[v, d], p), and the 64 lane sums are added by the xor butterfly (distances 32, 16,
 *             8, 4, 2, 1).  Against exact arithmetic |s_e - s| <= (D + 3) 2^-24 sum_d |H[u, d] R[t, d] H[v, d]|.
 *
 * tfgnn_distmult_ce_metrics: scores, weighted sigmoid cross-entropy, confusion counts and d loss / d score.  The label of
 * triple e is the fp32 d_labels[e * ld_labels], its weight w_e the fp32 d_weights[e * ld_weights], or 1 when d_weights is
 * NULL (element strides, as in tfgnn_softmax_ce_metrics).  d_workspace: tfgnn_distmult_ce_workspace_bytes() bytes, 8-byte
 * aligned.
 *   counted   triple e is counted iff w_e > 0 and y_e is exactly 0 or 1.  Any other label, and a zero, negative or NaN
 *             weight, make it uncounted: it adds nothing to any sum and its d_gscore entry is exactly 0; its score is still
 *             written.
 *   W         sum of w_e over the counted triples, added in double in a fixed order.
 *   loss      d_metrics[0] = sum over counted e of w_e (max(s, 0) - s y + log1pf(expf(-|s|))) / W: the element in fp32
 *             ([ext] tf.nn.sigmoid_cross_entropy_with_logits, as tfgnn_sigmoid_ce_metrics), times w_e and added in double.
 *             W == 0 (nothing counted): loss = 0 and every d_gscore entry is 0.
 *   scores    d_scores (optional, [N]) = s_e.
 *   counts    d_counts (optional, int64 [4]) = {tp, fp, tn, fn} over the counted triples with the prediction s > 0: a score
 *             of exactly 0 (and a NaN score) predicts 0.  d_metrics[1] = accuracy = (tp + tn) / counted, 0 / 0 -> nan.
 *   gradient  d_gscore (optional, [N]) = (w_e / W) (sigmoid(s_e) - y_e) for counted e, w_e / W formed in double and rounded
 *             to fp32, sigmoid(s) = 1 / (1 + expf(-s)).
 *   NaN       a NaN score of a counted triple makes the loss NaN; it is not hidden.
 * Three launches: (1) a weight pass reduces W and the number of counted triples to at most 64 partials; (2) the main pass,
 * one wave per triple - every wave adds those partials up in the same order, so every gradient is scaled by the same W -
 * leaves one partial per workgroup; (3) the fixed-order final stage.  d_metrics and d_counts are bit-identical run to run
 * and whether or not d_scores / d_counts / d_gscore are requested.
 * Refused: N < 1 ("empty batch"), N > 2^30, D outside [1, 1024], V or T outside [1, 2^31), ld_H < D, NULL d_H / d_R /
 * d_triples / d_labels / d_metrics, an element stride < 1, a short or misaligned workspace.
 *
 * Triple tables (int32, built on the host: ops.build_triple_tables):
 *   d_node_offsets [V + 1], d_node_entries [2 N]: node v owns the entries node_offsets[v] .. node_offsets[v + 1]; an entry is
 *     2 e + role, role 0: v is the source of triple e, role 1: v is its target; ascending within a node; a self triple
 *     (u == v) appears twice under u.  node_offsets[V] = 2 N (read as unsigned: 2^31 at N = 2^30).
 *   d_rel_offsets [T + 1], d_rel_order [N]: the triple ids grouped by relation, ascending within a relation.
 *
 * tfgnn_distmult_backward: from g = d_gscore [N],
 *   dH[v, d] = sum over the entries of v, ascending, of g_e R[t_e, d] H[other end of e, d]       (d_dH, row stride ld_dH >= D;
 *              columns >= D are not touched; a node without entries gets an exact 0 row; accumulate != 0: the sum is added
 *              to what d_dH holds, dH = dH + sum)
 *   dR[t, d] = sum over the triples of relation t in rel_order of g_e H[u_e, d] H[v_e, d]        (d_dR [T, D] contiguous; a
 *              relation without triples gets an exact 0 row)
 * Either output may be NULL (with its tables), not both.  A term is added as acc = fma(g_e * x[d], y[d], acc) with
 * (x, y) = (R[t_e], H[other end]) for dH and (H[u_e], H[v_e]) for dR.  SUM ORDER, the same rule for both: a row (node or
 * relation) of at most 256 list positions is added in list order starting from 0.  A longer row is cut into chunks of 256
 * consecutive positions counted from the row's start; every chunk is added in list order starting from 0 (first stage: one
 * wave per chunk, so a hub node of thousands of entries is spread over as many waves as it has chunks), and the chunk sums
 * are added in ascending chunk order starting from 0 (second stage).  The order depends on the tables alone.  Four
 * launches (two per requested gradient).  d_workspace: tfgnn_distmult_backward_workspace_bytes(N, D) bytes, 4-byte aligned.
 * Refused: as above, and NULL d_gscore, both outputs NULL, a requested gradient without its tables, ld_dH < D.
 *
 * tfgnn_distmult_rank: for each of Q queries (u, t, v) and side = 0 (corrupt the target: candidates (u, t, c)) or side = 1
 * (corrupt the source: (c, t, v)), over all candidate entities c in [0, V) scored with the same routine:
 *   d_greater[q] (int32 [Q]) = number of candidates with score >  the true triple's score,
 *   d_equal[q]   (int32 [Q]) = number of candidates with score == it,
 * both without the true entity itself (v for side 0, u for side 1) and without the ids of the optional filter:
 * d_filter_offsets int32 [Q + 1], d_filter_ids sorted and unique within a query, each in [0, V); the filter may or may not
 * contain the true entity.  Both NULL: no filter.  A NaN score compares false both ways.  The rank with ties split evenly is
 * 1 + greater + equal / 2 (utils/eval_metrics.py ranking_metrics).  Launches: a pre-pass, one wave per query, writes the
 * true score and MINUS the counts over the query's filter ids; the main pass - a workgroup per (candidate slice, tile of 16
 * queries), each wave reading a candidate's row once for the 16 queries - adds its counts with integer atomics, exact in any
 * order.  d_workspace: tfgnn_distmult_rank_workspace_bytes(Q) bytes, 4-byte aligned.  Refused: Q < 1 or > 2^30, a side other
 * than 0 / 1, one filter array without the other, and the size / pointer rules above.
 *
 * tfgnn_link_launch_counts: kernel launches so far of {tfgnn_distmult_ce_metrics, tfgnn_distmult_backward,
 * tfgnn_distmult_rank} (host counters; entries beyond the third are 0). */
size_t tfgnn_distmult_ce_workspace_bytes(void);
int tfgnn_distmult_ce_metrics(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_triples, const float* d_labels,
                              int64_t ld_labels, const float* d_weights, int64_t ld_weights, int64_t V, int64_t T, int64_t N,
                              int64_t D, float* d_metrics, int64_t* d_counts, float* d_scores, float* d_gscore,
                              void* d_workspace, size_t workspace_bytes, void* stream);
size_t tfgnn_distmult_backward_workspace_bytes(int64_t N, int64_t D);
int tfgnn_distmult_backward(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_triples, const float* d_gscore,
                            const int32_t* d_node_offsets, const int32_t* d_node_entries, const int32_t* d_rel_offsets,
                            const int32_t* d_rel_order, int64_t V, int64_t T, int64_t N, int64_t D, float* d_dH, int64_t ld_dH,
                            int accumulate, float* d_dR, void* d_workspace, size_t workspace_bytes, void* stream);
size_t tfgnn_distmult_rank_workspace_bytes(int64_t Q);
int tfgnn_distmult_rank(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_queries, int64_t Q, int side,
                        const int32_t* d_filter_offsets, const int32_t* d_filter_ids, int64_t V, int64_t T, int64_t D,
                        int32_t* d_greater, int32_t* d_equal, void* d_workspace, size_t workspace_bytes, void* stream);
int tfgnn_link_launch_counts(int64_t* out_counts, int n);

/* ------------------------------------------------------------------------------------------
 * Link prediction with a ComplEx decoder (LinkPredictionTask link_decoder="complex", csrc/link.hip; Trouillon et al. 2016; the
 * reference has no counterpart, PARITY UNPINNED).  DistMult is symmetric in its two entities; ComplEx is not.  D is even,
 * m = D / 2, and a row x of H or R is the complex vector x_re = x[0 .. m), x_im = x[m .. D): HALVES, not interleaved, so a
 * wave's loads of either part are coalesced.  For a triple (u, t, v) with a = H[u], r = R[t], b = H[v]:
 *   s = Re sum_k a[k] r[k] conj(b[k])
 *     = sum_k r_re[k] (a_re[k] b_re[k] + a_im[k] b_im[k]) + r_im[k] (a_re[k] b_im[k] - a_im[k] b_re[k])
 * The three calls have the parameter lists of their tfgnn_distmult_* namesakes (the rank workspace size also takes D) and
 * everything said there to be common holds here: d_H [V, D] with row stride ld_H >= D, d_R [T, D] contiguous, int32 [N, 3]
 * triples, the same triple tables, indices and tables NOT checked by the kernels, no allocation, no host synchronisation,
 * capturable on the one stream given, no floating-point atomic - every floating-point sum has an order that is a function
 * of the arguments and tables only, not of timing and not of which optional outputs are requested.  2 <= D <= 1024, D even
 * (an odd D is refused: "must be even"), 1 <= V, T < 2^31, 1 <= N <= 2^30.  Bad arguments are refused before any launch, by
 * the rules and with the messages of the DistMult calls.
 *   score     s_e in fp32 by ONE device routine shared by the kernels of tfgnn_complex_ce_metrics: lane l of a wave adds the
 *             complex columns k = l, l + 64, l + 128, ... in ascending order, per column
 *               x = fma(a_im, b_im, a_re * b_re);  y = fma(-a_im, b_re, a_re * b_im);  p = fma(r_re, x, p);  p = fma(r_im, y, p)
 *             and the 64 lane sums are added by the xor butterfly (distances 32, 16, 8, 4, 2, 1).  Against exact arithmetic
 *             |s_e - s| <= (2 D + 3) 2^-24 P_e, P_e = sum_k |r_re| (|a_re b_re| + |a_im b_im|) + |r_im| (|a_re b_im| + |a_im b_re|).
 *
 * tfgnn_complex_ce_metrics: tfgnn_distmult_ce_metrics with that score.  Counted triples, W, the loss element, the counts, the
 * s > 0 prediction, d_gscore, the NaN rule, the three launches and the bit-identity of d_metrics / d_counts whatever optional
 * outputs are requested are those of the DistMult call - it is the same code.  d_workspace:
 * tfgnn_complex_ce_workspace_bytes() bytes, 8-byte aligned.
 *
 * tfgnn_complex_backward: from g = d_gscore [N], over the same tables in the same SUM ORDER as tfgnn_distmult_backward (rows
 * of at most 256 list positions in list order, longer rows in chunks of 256 - one wave per chunk - and the chunk sums in
 * ascending chunk order), four launches (two per requested gradient), the same accumulate rule, exact 0 rows for a node or a
 * relation without entries, columns >= D of d_dH untouched.  The term of a list position, with role 0: the node is the
 * source a of the triple, role 1: it is the target b,
 *   dH_re += g (r_re b_re + r_im b_im)   dH_im += g (r_re b_im - r_im b_re)      (role 0)
 *   dH_re += g (r_re a_re - r_im a_im)   dH_im += g (r_re a_im + r_im a_re)      (role 1)
 *   dR_re += g (a_re b_re + a_im b_im)   dR_im += g (a_re b_im - a_im b_re)
 * is added as two fused multiply-adds per part.  With (x, y) = (R[t_e], H[other end]) for dH and (H[u_e], H[v_e]) for dR,
 * gr = g_e * x_re, gi = g_e * x_im, and sg = -gi for a role-1 entry of dH, gi otherwise:
 *   acc_re = fma(gr, y_re, acc_re);  acc_re = fma(sg, y_im, acc_re);  acc_im = fma(gr, y_im, acc_im);  acc_im = fma(-sg, y_re, acc_im)
 * A wave holds 256 complex columns at a time, re and im of a column in the same lane, so the four row reads of a term serve
 * both parts.  d_workspace: tfgnn_complex_backward_workspace_bytes(N, D) bytes, 4-byte aligned.
 *
 * tfgnn_complex_rank: the outputs, the filter semantics and the NaN rule of tfgnn_distmult_rank; the counts are exact integers
 * (integer atomics).  The score of a candidate is linear in its row, so the pre-pass (one wave per query) writes one QUERY
 * VECTOR q [D] per query into the workspace,
 *   side 0, candidates (u, t, c):  q_re = fma(r_re, a_re, -(r_im * a_im))   q_im = fma(r_re, a_im, r_im * a_re)
 *   side 1, candidates (c, t, v):  q_re = fma(r_re, b_re, r_im * b_im)      q_im = fma(r_re, b_im, -(r_im * b_re))
 * and EVERY score of the call - the true triple's (the true entity's row as the candidate), the filter ids', the candidates' -
 * is the dot product <q, H[c]> by one routine: lane l adds d = l, l + 64, ... in ascending order as p = fma(q[d], H[c, d], p),
 * then the butterfly.  A candidate whose row equals the true entity's bit for bit therefore counts as equal.  These scores are
 * NOT the bits of tfgnn_complex_ce_metrics (another operation order); they lie within the same (2 D + 3) 2^-24 P_e of exact
 * arithmetic.  Launches: the pre-pass (query vectors, true scores, MINUS the counts over the filter ids) and the main pass - a
 * workgroup per (candidate slice, tile of 16 queries), each wave scoring its LDS-resident candidate row against the 16 query
 * vectors.  d_workspace: tfgnn_complex_rank_workspace_bytes(Q, D) = Q (D + 1) floats, 4-byte aligned.
 *
 * The *_workspace_bytes(..) calls return 0 for sizes the calls refuse (D odd or outside [2, 1024], N or Q outside [1, 2^30]).
 * tfgnn_complex_launch_counts: kernel launches so far of {tfgnn_complex_ce_metrics, tfgnn_complex_backward,
 * tfgnn_complex_rank} (host counters; entries beyond the third are 0).  tfgnn_link_launch_counts counts the DistMult calls
 * only. */
size_t tfgnn_complex_ce_workspace_bytes(void);
int tfgnn_complex_ce_metrics(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_triples, const float* d_labels,
                             int64_t ld_labels, const float* d_weights, int64_t ld_weights, int64_t V, int64_t T, int64_t N,
                             int64_t D, float* d_metrics, int64_t* d_counts, float* d_scores, float* d_gscore,
                             void* d_workspace, size_t workspace_bytes, void* stream);
size_t tfgnn_complex_backward_workspace_bytes(int64_t N, int64_t D);
int tfgnn_complex_backward(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_triples, const float* d_gscore,
                           const int32_t* d_node_offsets, const int32_t* d_node_entries, const int32_t* d_rel_offsets,
                           const int32_t* d_rel_order, int64_t V, int64_t T, int64_t N, int64_t D, float* d_dH, int64_t ld_dH,
                           int accumulate, float* d_dR, void* d_workspace, size_t workspace_bytes, void* stream);
size_t tfgnn_complex_rank_workspace_bytes(int64_t Q, int64_t D);
int tfgnn_complex_rank(const float* d_H, int64_t ld_H, const float* d_R, const int32_t* d_queries, int64_t Q, int side,
                       const int32_t* d_filter_offsets, const int32_t* d_filter_ids, int64_t V, int64_t T, int64_t D,
                       int32_t* d_greater, int32_t* d_equal, void* d_workspace, size_t workspace_bytes, void* stream);
int tfgnn_complex_launch_counts(int64_t* out_counts, int n);

/* ------------------------------------------------------------------------------------------
 * Negative sampling and triple tables on the device (csrc/negatives.hip): what LinkPredictionDataset does per epoch on the
 * host - draw the negatives, rebuild the triple tables - as calls on the caller's stream, so that a captured training step
 * carries its own fresh negatives.  Integers only: no call does float arithmetic.  No call allocates or synchronises with
 * the host; both are capturable.  Bad arguments are refused before any launch.  The kernels do not validate indices: the
 * positives are validated on the host when they are loaded, the negatives are in range by construction.
 *
 * tfgnn_triples_draw_negatives: d_triples int32 [N, 3], N = P (1 + K); rows 0 .. P - 1 are the positives and are only read,
 * rows P .. N - 1 are written, each whole row (u, t, v), so the buffer needs no initial content beyond the positives.
 *   order     negative j (0 <= j < P K) copies positive j / K (np.repeat order) and replaces its source or its target with
 *             a node drawn from the OTHER V - 1 nodes: exactly one slot differs, the relation is kept.  Negatives are not
 *             filtered against known triples.
 *   numbers   "The dropout mask generator" above, nothing else: with word(g) as defined there for (seed, epoch),
 *               a = word(2 j), b = word(2 j + 1)        (2 j + 1 < 2^31: the high-word term h is always 0)
 *               slot = the target if a >> 31, else the source
 *               draw = ((uint64) b * (V - 1)) >> 32      (the multiply-high draw, in [0, V - 1))
 *               new node = draw + (draw >= old node)     (skips the old node: in [0, V), never the old one)
 *             Bias of the multiply-high draw: value d is taken by floor or ceil of 2^32 / (V - 1) of the 2^32 words b, so
 *             every node's probability is within 2^-32 of 1 / (V - 1): a relative bias of at most (V - 1) / 2^32.
 *   epoch     use_epoch != 0: the kernel reads the dropout epoch word once when it starts, like every kernel that draws a
 *             mask, so a step replayed from a captured hipGraph after tfgnn_dropout_epoch_advance redraws at every replay.
 *             use_epoch == 0: the word is ignored (the key of epoch 0): a fixed draw whatever the epoch.
 * One launch; K == 0 (N == P) is accepted and launches nothing.  Refused: P < 1, N outside [1, 2^30], K < 0 or
 * N != P (1 + K), NULL d_triples, V outside [1, 2^31), V < 2 with K > 0.
 *
 * tfgnn_triple_tables_build: the "Triple tables" above from DEVICE triples [N, 3] - exactly the arrays
 * ops.build_triple_tables builds on the host: node_entries = the positions 2 e + role stably sorted by the node in that
 * role, rel_order = the triple ids stably sorted by relation (ascending within a node / a relation), the offsets their row
 * pointers, stored as unsigned words (node_offsets[V] = 2^31 at N = 2^30).  Either pair (d_node_offsets with
 * d_node_entries, d_rel_offsets with d_rel_order) may be NULL, not both: a NULL pair is neither built nor touched.  The
 * tables are a function of the triples alone: a stable LSD radix sort with 9-bit digits over per-tile histograms (the scheme
 * of csrc/graph.hip), no global atomic, LDS integer atomics only for histogram counts.  A node that owns most of the entries
 * is many equal keys of the sort, not a row some wave walks.
 *   launches  passes(X) = max(1, ceil(ceil(log2 X) / 9)) digit passes for keys in [0, X), two launches each (histogram,
 *             scatter), and one launch for the row pointers:
 *               node pair 2 passes(V) + 1,  relation pair 2 passes(T) + 1,  both: the sum.   A function of (V, T) and of
 *             which pairs are requested - not of N, not of the data.
 *   workspace tfgnn_triple_tables_workspace_bytes(N, V, T) bytes (0 for sizes the build refuses), 16-byte aligned:
 *             two key and two payload arrays of 2 N words and the [512][tiles] histogram table, tiles = ceil(2 N / 8192).
 *             A scatter workgroup reads the table's tile columns up to its own, so a pass costs O(tiles^2) table words next to
 *             the O(N) keys: 0.2 M words per workgroup at N = 1.4 M.
 * Refused: N < 1 ("empty batch"), N > 2^30, V or T outside [1, 2^31), NULL d_triples, half a pair, both pairs NULL, a short
 * or misaligned workspace.
 *
 * tfgnn_negatives_launch_counts: kernel launches so far of {tfgnn_triples_draw_negatives, tfgnn_triple_tables_build} (host
 * counters; entries beyond the second are 0). */
int tfgnn_triples_draw_negatives(int32_t* d_triples, int64_t N, int64_t P, int64_t K, int64_t V, uint64_t seed, int use_epoch,
                                 void* stream);
size_t tfgnn_triple_tables_workspace_bytes(int64_t N, int64_t V, int64_t T);
int tfgnn_triple_tables_build(const int32_t* d_triples, int64_t N, int64_t V, int64_t T, int32_t* d_node_offsets,
                              int32_t* d_node_entries, int32_t* d_rel_offsets, int32_t* d_rel_order, void* d_workspace,
                              size_t workspace_bytes, void* stream);
int tfgnn_negatives_launch_counts(int64_t* out_counts, int n);

/* ------------------------------------------------------------------------------------------
 * Layer-level entry points (round 6): one call per message-passing layer and pass.
 * Replaces, for one layer, MessagePassing.call (message_passing.py:95-133) with
 * _calculate_messages_per_type (:181-218), GNN_Edge_MLP._message_function (gnn_edge_mlp.py:84-107) and
 * _compute_new_node_embeddings (message_passing.py:135-179) - and their share of tape.gradient
 * (models/graph_task_model.py:347-357) - in the aggregate-first formulation on split operands, the route of RGCN, of
 * GGNN's message part and of GNN_Edge_MLP without hidden layers / target states (sum, mean or sqrt_n aggregation, activation
 * after aggregation; hidden_dim and in_dim multiples of 128 or of 320).  Each function enqueues, on `stream`, exactly the
 * kernels the op-level calls named below would: results are bit-identical to that route.
 *
 * All pointers are device pointers unless named h_*; buffers are the caller's (sizes in comments, V = nodes, L = edge types
 * of the graph handle, D = in_dim, H = hidden_dim).  `struct_size` = sizeof of the struct (a binding built against another
 * header is rejected).
 * ------------------------------------------------------------------------------------------ */
typedef enum {
  TFGNN_MP_AGGREGATE_FIRST = 0 /* linear message per edge type, aggregated before the per-relation product */
} tfgnn_mp_kind;

typedef struct tfgnn_mp_forward_args {
  size_t struct_size;
  int kind; /* tfgnn_mp_kind */
  const tfgnn_graph* graph;
  int view;                 /* TFGNN_VIEW_BY_DST_TYPED, or ..._PATTERN with tile_kmask / row_map of the handle */
  const float* x;           /* node states [V, D], row pitch ldx floats */
  int64_t ldx;
  int in_dim, hidden_dim;
  const float* row_scale;   /* [V * L] factor per (node, type) bucket - 1 / (c + 1e-7), tfgnn_graph_scales - or NULL */
  const float* w;           /* stacked kernels [L * D, H] row-major: non-NULL = (re)build the operand below from them (a
                             * small-pass launch between the gather and the product).  A stack of layers does better to
                             * split all its stale weights in ONE tfgnn_aux_launch at the start of the pass - the weights do
                             * not change before the optimizer update - and to pass NULL here */
  void* wt_sp;              /* W^T as SP16 [H, L * D] (row pitch ld_wt_sp_bytes) + wt_inv_scale [H]: kept by the caller */
  int64_t ld_wt_sp_bytes;   /*   across calls while the kernels do not change                                          */
  float* wt_inv_scale;
  void* agg_sp;             /* scratch: the aggregate [V, L * D] SP16 (V * L * D * 4 bytes) + agg_inv_scale [V * L] */
  float* agg_inv_scale;
  const float* bias;        /* [H] or NULL */
  int act;                  /* tfgnn_activation applied to the sum (message_passing.py:176-177) */
  float dropout_rate;       /* > 0: the NEXT op's input dropout applied to the result (tfgnn_sp_gemm_nt_dropout) */
  uint64_t dropout_seed;
  const uint8_t* tile_kmask; /* TFGNN_G_PATTERN_TILEMASK_BY_DST with the PATTERN view, else NULL */
  const int32_t* row_map;    /* TFGNN_G_PATTERN_NODE_BY_DST with the PATTERN view, else NULL */
  float* out;               /* [V, H] fp32, row pitch ld_out floats (may be NULL when out_sp is given) */
  int64_t ld_out;
  void* out_sp;             /* optional: the result as a split operand [V, H] + out_inv_scale [V * (H / tile width)] */
  int64_t ld_out_sp_bytes;
  float* out_inv_scale;
  void* workspace;          /* tfgnn_graph_gather_workspace_bytes(graph, view, D) bytes */
  size_t workspace_bytes;
  int agg_filled;           /* != 0: agg_sp / agg_inv_scale already hold the empty buckets' rows of this graph and view (same D,
                             * same row_scale values, written by an earlier call and untouched since): the gather leaves them
                             * alone - keep_empty_rows of tfgnn_graph_gather_reduce_sp_keep_empty, with its contract.  0: every
                             * row is written.  A caller that keeps the pair with the graph sets it from the second layer on */
} tfgnn_mp_forward_args;

typedef struct tfgnn_mp_backward_args {
  size_t struct_size;
  int kind;
  const tfgnn_graph* graph;
  const float* d_pre;       /* gradient w.r.t. the layer's pre-activation sums [V, H], row pitch ld_d_pre floats */
  int64_t ld_d_pre;
  int in_dim, hidden_dim;
  const float* edge_weight; /* [E] factor per edge in by-source order (tfgnn_graph_scales d_edge_weight_by_src) or NULL */
  const float* w;           /* stacked kernels [L, D, H]: non-NULL = (re)build the operand below */
  void* wh_sp;              /* rows [W_0[d, :] | W_1[d, :] | ..] as SP16 [D, L * H] + wh_inv_scale [D] */
  int64_t ld_wh_sp_bytes;
  float* wh_inv_scale;
  void* g_sp;               /* scratch: G [V, L * H] SP16 + g_inv_scale [V * L] */
  float* g_inv_scale;
  /* d(node states) = epilogue(G W^T): fp32 result dx [V, D] (added into when accumulate), times mul [V, D] (NULL: 1), times
   * act'(saved * saved_scale) of activation act_of_saved (saved NULL: 1), times the dropout mask of (rate, seed) (rate 0: none);
   * optionally also as a split operand */
  float* dx;
  int64_t ld_dx;
  int accumulate;
  const float* mul;
  int64_t ld_mul;
  int act_of_saved;
  const float* saved;
  int64_t ld_saved;
  float saved_scale;
  float dropout_rate;
  uint64_t dropout_seed;
  void* dx_sp;
  int64_t ld_dx_sp_bytes;
  float* dx_inv_scale;
  const uint8_t* tile_kmask; /* TFGNN_G_PATTERN_TILEMASK_BY_SRC + a_rows = row_map = TFGNN_G_PATTERN_NODE_BY_SRC, or all NULL */
  const int32_t* a_rows;
  const int32_t* row_map;
  /* kernel gradients dW [L, D, H] = X^T G_l (dw NULL: skipped): the layer input as a split operand [V, D], one scale per row */
  float* dw;
  const void* x_sp;
  int64_t ld_x_sp_bytes;
  const float* x_inv_scale;
  void* tn_workspace;       /* tfgnn_sp_gemm_tn_workspace_bytes(L * H, D, V, L * H, H) bytes, 256-byte aligned */
  size_t tn_workspace_bytes;
  void* workspace;          /* tfgnn_graph_gather_workspace_bytes(graph, TFGNN_VIEW_BY_SRC_TYPED, H) bytes */
  size_t workspace_bytes;
  /* Up to 1024 row tiles of 128 nodes the pass runs gather - weight-gradient product - input-gradient product, and the
   * latter's launch carries the reduce pass of the former (tfgnn_sp_gemm_nt_rows_tail): tn_workspace is read while the
   * input-gradient product runs.  tn_workspace may overlap neither workspace nor the K-split workspace of the NT product
   * (tfgnn_sp_gemm_nt_set_splitk_workspace); a call where it does is refused.  Over more nodes the order is gather - input-
   * gradient product - tfgnn_sp_gemm_tn, its reduce pass in its own launch.  Same results either way, bit for bit. */
  int g_filled;             /* != 0: g_sp / g_inv_scale already hold the empty buckets' rows of this graph's by-source view
                             * (same H; see agg_filled of tfgnn_mp_forward_args).  0: every row is written */
} tfgnn_mp_backward_args;

/* = tfgnn_graph_gather_reduce_sp_deferred + tfgnn_sp_split_cols_job + tfgnn_aux_launch + tfgnn_sp_gemm_nt_rows */
int tfgnn_mp_forward(const tfgnn_mp_forward_args* args, void* stream);
/* = tfgnn_graph_gather_reduce_sp_deferred + tfgnn_sp_split_rows_job + tfgnn_aux_launch + tfgnn_sp_gemm_tn_product +
 *   tfgnn_sp_gemm_nt_rows_tail */
int tfgnn_mp_backward(const tfgnn_mp_backward_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Graph readout (csrc/pool_fused.hip): the tail of WeightedSumGraphRepresentation.call behind its two MLPs
 * (nodes_to_graph_representation.py:170-229) - per-graph softmax of the scores (:178-186), clip of the transformed nodes
 * (:194-197), weighted segment sum (:204-227) - and its share of tape.gradient, one call each.  With h(f) = f / (GD / heads):
 *   out[g, f] = sum over the nodes v of graph g of  w[v, h(f)] * min(max(T[v, f], lo), hi)          (an empty graph: a zero row)
 *   TFGNN_POOL_SOFTMAX  w = exp(S - m_g) / (sum_g exp(S - m_g) + 1e-7) per (graph, head), what tfgnn_segment_softmax computes;
 *                       written to `w` (the backward call reads it)
 *   TFGNN_POOL_SIGMOID  w = S: the scoring MLP's final activation already applied the sigmoid; `w` is not written
 *   TFGNN_POOL_NONE     w = 1;   TFGNN_POOL_AVERAGE  w = 1 / max(number of nodes of g, 1)
 * backward:
 *   dT[v, f] = w[v, h(f)] * dOut[g, f] where lo <= T[v, f] <= hi, else 0                             (tfgnn_clip_backward's mask)
 *   dw[v, h] = sum over the features f of head h of clip(T[v, f]) * dOut[g, f]                       (never written to memory)
 *   SOFTMAX  dS[v, h] = w * (dw - sum over the graph of w * dw);   SIGMOID  dS = dw (pass w = S);   dS NULL: not computed
 * lo / hi: -INFINITY / +INFINITY for an absent bound.  T, S, w, dT, dS have leading dimensions (floats); out and dOut are
 * contiguous [G, GD]; ptr [G + 1] comes from tfgnn_segment_offsets*.  A NaN in T stays a NaN through the clip (it reaches
 * out and dS; the mask of dT is false there), +-inf in T clips to a finite bound: what tf.maximum / tf.minimum do.
 *
 * The nodes are cut into tiles of TFGNN_POOL_CHUNK_NODES; a graph with more nodes than that is reduced chunk by chunk by
 * several workgroups, whose partial results (in `workspace`) a second launch combines in ascending chunk order - no float
 * atomics, results independent of the grid and the run.  At most two launches per call; the second one only when
 * V > TFGNN_POOL_CHUNK_NODES (otherwise no graph can have been cut; workgroups whose tile holds no chunk leave at once), and
 * in the backward call only for SOFTMAX with dS.  No allocation, no synchronisation: capturable as they are.
 * Rejected on the host before any HIP call: a struct of another size, an unknown kind, negative sizes, heads that do not
 * divide GD, lo > hi, a workspace smaller than tfgnn_pool_workspace_bytes (which needs no device; 0 when
 * V <= TFGNN_POOL_CHUNK_NODES).  V == 0, G == 0 or GD == 0: nothing is launched (and nothing written), TFGNN_OK.
 * GD > 1024: TFGNN_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
#define TFGNN_POOL_CHUNK_NODES 128
typedef enum { TFGNN_POOL_SOFTMAX = 0, TFGNN_POOL_SIGMOID = 1, TFGNN_POOL_NONE = 2, TFGNN_POOL_AVERAGE = 3 } tfgnn_pool_kind;

typedef struct tfgnn_pool_forward_args {
  size_t struct_size;
  int kind; /* tfgnn_pool_kind */
  int64_t V, G;
  int GD, heads;
  const int32_t* ptr; /* [G + 1] */
  const float* T;     /* [V, GD], row pitch ldT: the transformation MLP's output after its activation, not clipped */
  int64_t ldT;
  const float* S;     /* [V, heads], row pitch ldS: scores (SOFTMAX) / sigmoid weights (SIGMOID); NULL for NONE, AVERAGE */
  int64_t ldS;
  float lo, hi;
  float* out;         /* [G, GD] */
  float* w;           /* [V, heads], row pitch ldw: written for SOFTMAX, otherwise unused (may be NULL) */
  int64_t ldw;
  void* workspace;    /* tfgnn_pool_workspace_bytes(V, G, GD, heads, kind) bytes, 16-byte aligned */
  size_t workspace_bytes;
} tfgnn_pool_forward_args;

typedef struct tfgnn_pool_backward_args {
  size_t struct_size;
  int kind;
  int64_t V, G;
  int GD, heads;
  const int32_t* ptr;
  const int32_t* ids; /* [V] node -> graph; the kernels find a node's graph through ptr, so this may be NULL */
  const float* dOut;  /* [G, GD] */
  const float* T;
  int64_t ldT;
  const float* w;     /* SOFTMAX: what the forward call wrote; SIGMOID: S; NULL for NONE, AVERAGE */
  int64_t ldw;
  float lo, hi;
  float* dT;          /* [V, GD], row pitch lddT */
  int64_t lddT;
  float* dS;          /* [V, heads], row pitch lddS; NULL = not wanted (must be NULL for NONE, AVERAGE) */
  int64_t lddS;
  void* workspace;    /* the same query as the forward call */
  size_t workspace_bytes;
} tfgnn_pool_backward_args;

size_t tfgnn_pool_workspace_bytes(int64_t V, int64_t G, int GD, int heads, int kind);
/* = tfgnn_segment_softmax + tfgnn_clip + tfgnn_segment_weighted_sum, on kernels of its own */
int tfgnn_pool_forward(const tfgnn_pool_forward_args* args, void* stream);
/* = tfgnn_segment_weighted_sum_backward + tfgnn_clip_backward + tfgnn_segment_softmax_backward, on kernels of its own */
int tfgnn_pool_backward(const tfgnn_pool_backward_args* args, void* stream);
/* host-side counts of the kernel launches the two calls have enqueued in this process: out[0] forward ("pool_fwd"),
 * out[1] backward ("pool_bwd"), the combining launches included; further slots are zero */
int tfgnn_pool_launch_counts(int64_t* out_counts, int n);

/* ------------------------------------------------------------------------------------------
 * Optimizer step (csrc/optim.hip): GraphTaskModel._apply_gradients (models/graph_task_model.py:279-324) with the optimizers
 * of _make_optimizer (:224-277) - [ext] TF 2.x optimizer_v2 arithmetic, fp32:
 *   SGD      momentum > 0: accum = accum * mu - lr * g;  w += accum          momentum 0: w -= lr * g
 *   RMSprop  momentum > 0: ms += (g^2 - ms)(1 - rho);  mom = mom * mu + lr * g * rsqrt(ms + eps);  w -= mom
 *            momentum 0:   ms = rho * ms + (1 - rho) g^2;  w -= lr * g / (sqrt(ms) + eps)          (non-centered)
 *   Adam     t = iterations + 1, alpha = lr * sqrt(1 - b2^t) / (1 - b1^t);
 *            m += (g - m)(1 - b1);  v += (g^2 - v)(1 - b2);  w -= m * alpha / (sqrt(v) + eps)
 * after clipping the gradients (:296-322): by value (clip_by_value), per-tensor norm (g * c / max(|g|, c)) or global norm
 * (g * c * min(1 / N, 1 / c), N the root of the sum of squares over every tensor of the call; N inf or NaN gives NaN).
 * The learning rate is computed ON THE DEVICE from the step counter `iterations` (state[0]): constant, or the polynomial
 * warm-up / decay schedule (utils/polynomial_warmup_and_decay_schedule.py:90-111) at step = (float)iterations, in fp32.
 * Every call advances the counter once, so a call captured into a hipGraph follows the schedule on every replay.
 *
 * One call updates every tensor given to it: one launch per chunk of 32 tensors, and with a norm mode first one more launch
 * per chunk that writes per-workgroup partial sums of squares to the workspace (reduced in a fixed order by the update:
 * bit-reproducible, no float atomics).  The counter is advanced by the last workgroup to finish the last update launch
 * (an integer ticket in state[1]), after every workgroup of the call has read it.
 * ------------------------------------------------------------------------------------------ */
typedef enum { TFGNN_OPT_SGD = 0, TFGNN_OPT_RMSPROP = 1, TFGNN_OPT_ADAM = 2 } tfgnn_opt_kind;
typedef enum { TFGNN_CLIP_NONE = 0, TFGNN_CLIP_VALUE = 1, TFGNN_CLIP_NORM = 2, TFGNN_CLIP_GLOBAL_NORM = 3 } tfgnn_clip_mode;
/* one variable and its gradient as 2-D row-major views (a 1-D tensor is one row): element (r, c) at value[r * ld_value + c] and
 * grad[r * ld_grad + c], so column slices of a fused buffer are described in place.  The slots are contiguous [rows * cols]
 * fp32 arrays owned by the optimizer, zero before the first call: SGD slot0 = accumulator (momentum > 0 only); RMSprop
 * slot0 = mean square, slot1 = momentum (momentum > 0 only); Adam slot0 = m, slot1 = v.  Unused slots may be NULL. */
typedef struct tfgnn_opt_tensor {
  float* value;
  int64_t ld_value;
  const float* grad;
  int64_t ld_grad;
  int64_t rows;
  int64_t cols;
  float* slot0;
  float* slot1;
} tfgnn_opt_tensor;
typedef struct tfgnn_opt_config {
  size_t struct_size; /* sizeof(tfgnn_opt_config) */
  int kind;           /* tfgnn_opt_kind */
  int clip;           /* tfgnn_clip_mode */
  float clip_value;   /* > 0 when clip != TFGNN_CLIP_NONE */
  float momentum;     /* SGD, RMSprop: in [0, 1] */
  float rho;          /* RMSprop */
  float beta_1, beta_2, epsilon; /* Adam (beta_*), RMSprop and Adam (epsilon) */
  int schedule;       /* 0: constant learning_rate; 1: polynomial warm-up and decay */
  float learning_rate, initial_learning_rate, final_learning_rate, power;
  int64_t warmup_steps, decay_steps;
  int64_t* state;     /* device, 16 bytes, zero-initialised: [0] iterations, [1] ticket of the last update launch */
  void* workspace;    /* tfgnn_optimizer_workspace_bytes(...) bytes (norm modes), 16-byte aligned */
  size_t workspace_bytes;
} tfgnn_opt_config;
size_t tfgnn_optimizer_workspace_bytes(const tfgnn_opt_tensor* tensors, int n, int clip);
int tfgnn_optimizer_apply(const tfgnn_opt_tensor* tensors, int n, const tfgnn_opt_config* config, void* stream);
/* state[0] -> *out (device or host-mapped memory) / state[0] = value, state[1] = 0: one-thread kernels, capturable */
int tfgnn_optimizer_iterations_get(const int64_t* state, int64_t* out, void* stream);
int tfgnn_optimizer_iterations_set(int64_t* state, int64_t value, void* stream);
/* host-side count of the kernel launches tfgnn_optimizer_apply and tfgnn_optimizer_apply_rows have enqueued in this process
 * (tests) */
int64_t tfgnn_optimizer_launch_count(void);

/* The row-sparse ("lazy") step: the same update for variables whose gradient is a ROW GRADIENT - the pair (grad_rows [n, cols],
 * ids [n]) against a table of N rows, standing for the dense gradient that is grad_rows[i] at row ids[i] and zero elsewhere
 * (the gradient of tfgnn_gather_node_rows; the ids are DISTINCT by precondition, as for tfgnn_embedding_scatter_rows).
 *
 *   listed rows      value[ids[i], :] and the slots at those rows get exactly the arithmetic of the dense step: the same
 *                    clipping, the learning rate from the device counter, Adam's alpha at t = iterations + 1.
 *   all other rows   neither their value nor their slots are read or written.
 *
 * So plain SGD (momentum 0) equals the dense step on the dense gradient; SGD with momentum, RMSprop and Adam are the LAZY
 * variant of the optimizer (LazyAdam / SparseAdam): the moments of rows without a gradient do not decay, and those rows do not
 * move.  An id outside [0, N) skips its row and sets *bad_flag (nullable, zeroed by the caller).  With a repeated id the result
 * of its row is unspecified; nothing else is affected.
 *
 * One call updates `n` dense tensors and `n_rows` row tensors (at most TFGNN_OPT_MAX_ROW_TENSORS) together:
 *   counter   state[0] advances exactly once, after every workgroup of the call has read it: the ticket is taken in the LAST
 *             launch of the call - the row update, or the last dense update when every row tensor has n == 0 (such a call
 *             still updates its dense tensors and still advances the counter; no empty grid is launched - a call with nothing
 *             at all to update advances the counter with one workgroup).
 *   norms     in the norm modes a row tensor takes part in the squared-sum pass as the plain [n, cols] tensor grad_rows is,
 *             after every dense tensor of the call, in the same 8192-element partition: its per-tensor norm and the global
 *             norm are those of the dense gradient it stands for, and the bits of a tfgnn_optimizer_apply call that lists
 *             grad_rows as the gradient of a contiguous, aligned [n, cols] variable in that position.  A row skipped for a
 *             bad id still counts (the flag already says that the step is wrong).
 *   launches  the dense tensors as in tfgnn_optimizer_apply, then ONE launch for all row tensors; in the norm modes the row
 *             tensors' partial sums ride in the squared-sum launch of the last chunk of dense tensors.  32 dense tensors or
 *             fewer and row tensors: 2 launches, 3 with a norm mode.
 *   kernel    min(256, 8192 / cols) rows (one when a row is longer) to a workgroup; one thread per row checks the id and
 *             leaves it in LDS, then consecutive lanes walk consecutive floats of a row: per element w, g, slot0, slot1 are
 *             read and w, slot0, slot1 written.  float4 when cols % 4 == 0, both pitches are multiples of 4 and every base
 *             is 16-byte aligned; otherwise scalar accesses, four consecutive elements of the [n, cols] gradient's flat index
 *             space to a thread and its last n * cols % 4 elements one to a thread - the partition in which
 *             tfgnn_optimizer_apply computes that tensor, so that the two agree bit for bit at every shape.  Table and slot
 *             offsets are 64-bit: N * cols may pass 2^31 (tfgnn_optimizer_apply refuses such a tensor).  Plain stores, no
 *             float atomics.
 * No synchronisation, allocation or copy: capturable.  Rejected on the host before any HIP call: what tfgnn_optimizer_apply
 * rejects for the config and the dense tensors; for a row tensor negative sizes, cols < 1, N or cols >= 2^31, n > N,
 * n * cols >= 2^31 (grad_rows is an ordinary tensor of the squared-sum pass), a pitch below cols or (ld_grad) >= 2^32, and for
 * n > 0 a NULL value, grad_rows, ids or slot the optimizer kind needs. */
#define TFGNN_OPT_MAX_ROW_TENSORS 8
typedef struct tfgnn_opt_row_tensor {
  float* value;           /* the table [N, cols], row pitch ld_value >= cols */
  int64_t ld_value;
  const float* grad_rows; /* [n, cols], row pitch ld_grad >= cols */
  int64_t ld_grad;
  const int32_t* ids;     /* [n], distinct */
  int64_t n, N, cols;     /* 0 <= n <= N < 2^31, 1 <= cols < 2^31; N * cols may exceed 2^31 */
  float* slot0;           /* contiguous [N * cols], as in tfgnn_opt_tensor; unused may be NULL */
  float* slot1;
  int* bad_flag;          /* may be NULL */
} tfgnn_opt_row_tensor;
size_t tfgnn_optimizer_rows_workspace_bytes(const tfgnn_opt_tensor* tensors, int n, const tfgnn_opt_row_tensor* row_tensors,
                                            int n_rows, int clip);
int tfgnn_optimizer_apply_rows(const tfgnn_opt_tensor* tensors, int n, const tfgnn_opt_row_tensor* row_tensors, int n_rows,
                               const tfgnn_opt_config* config, void* stream);

/* ------------------------------------------------------------------------------------------
 * Batch assembly from a device-resident fold (csrc/batch.hip): GraphDataset.graph_batch_iterator_from_graph_iterator
 * (data/graph_dataset.py:161-246) for a fold whose graphs were packed onto the device once.
 *
 * Fold store (N graphs, laid end to end in file order; plain device arrays the caller owns):
 *   node_ptr [N + 1]              nodes before graph i;  features [store_nodes, F] fp32, store_nodes = node_ptr[N] < 2^31
 *   per processed edge type t:    edge_ptr[t] [N + 1] edges of type t before graph i;  edges[t] [edge_ptr[t][N], 2] int32,
 *                                 rows (src, dst) with graph-LOCAL node ids, in the order the reference gives them
 *   per column c:                 columns[c] [N] fp32, one value per graph (target_value, ...)
 *   per node column c:            node_columns[c] [store_nodes, W_c] fp32, one row per node, laid out like `features`, every
 *                                 column with its own width W_c = node_column_widths[c] (node_labels, ...)
 * Epoch arrays (uploaded once per epoch; P = order_len positions):
 *   order [P]                     graph id at position p (any ids in [0, N), repeats allowed)
 *   pos_node_ptr [P + 1]          nodes of the graphs at positions 0 .. p-1;  pos_edge_ptr[t] [P + 1] likewise per type
 * The call assembles the batch of positions [p0, p1), G = p1 - p0 graphs, with i = p - p0:
 *   node_features[pos_node_ptr[p] - pos_node_ptr[p0] + j, :] = features[node_ptr[order[p]] + j, :]
 *   node_to_graph_map[the same row]                           = i
 *   adjacency_lists[t][pos_edge_ptr[t][p] - pos_edge_ptr[t][p0] + k] = edges[t][edge_ptr[t][order[p]] + k] + (that node offset)
 *   column_out[c][i]                                          = columns[c][order[p]]
 *   node_column_out[c][pos_node_ptr[p] - pos_node_ptr[p0] + j, :] = node_columns[c][node_ptr[order[p]] + j, :]
 * The caller keeps the per-graph counts on the host, so it knows - and passes - the output sizes: num_nodes = V and
 * num_edges[t] = E_t; it allocates the outputs.  The kernel never writes past them: a size that disagrees with the device's
 * prefix sums, a graph id outside [0, N) or a local node id outside its graph sets *bad_flag (nullable, zeroed by the caller)
 * and the element is skipped or, for a bad local id, written as computed - what tfgnn_batch_offset_edges does.
 *
 * ONE launch per call, its grid partitioned over the parts (feature tiles, which also write node_to_graph_map; the tiles
 * of every node column; every edge type; the columns); none when the batch is empty (G == 0).  No copy, no allocation, no
 * synchronisation.  Feature and node column rows are copied with consecutive lanes on consecutive floats (per array: float4
 * when its width % 4 == 0 and both of its buffers are 16-byte aligned), rows_per_tile = clamp(8192 / width, 1, 256) rows to a
 * workgroup; element offsets into the store are 64-bit.  A node column row whose source disagrees with the store sizes is
 * skipped and sets *bad_flag, like a feature row; nothing is written beyond num_nodes rows.  Zero-length segments (no edges
 * of a type, no nodes) cost nothing.  With num_node_columns == 0 the grid and every output are what they are without them.
 * The pointer tables (edge_ptr, edges, pos_edge_ptr, adjacency_lists, num_edges, columns, column_out, node_column_widths,
 * node_columns, node_column_out) are HOST arrays of num_edge_types / num_columns / num_node_columns entries, read during the
 * call.
 * Rejected on the host before any HIP call: NULL args, another struct_size, negative sizes, p0 > p1 or p1 > order_len,
 * feature_dim < 1 or >= 2^31, store_nodes or num_nodes >= 2^31, num_edges[t] >= 2^31, NULL pointers where the size is not
 * zero, edge buffers that are not 8-byte aligned, a negative num_node_columns, a NULL node column table when there are node
 * columns, a node column width < 1 or >= 2^31, a NULL node column when num_nodes > 0.  More than TFGNN_BATCH_MAX_EDGE_TYPES
 * types, TFGNN_BATCH_MAX_COLUMNS columns or TFGNN_BATCH_MAX_NODE_COLUMNS node columns: TFGNN_ERR_UNSUPPORTED.
 * More than TFGNN_BATCH_MAX_EDGE_TYPES types: the caller chunks.  An edge tile reads pos_node_ptr and node_ptr, never
 * num_nodes, so a call with num_nodes = 0, num_columns = 0, num_node_columns = 0 and G > 0 launches edge tiles only (the
 * node outputs may be NULL; feature_dim still has to be >= 1).  A batch of L types is ceil(L / 48) calls on one stream with
 * the same bad_flag: the first carries the features, the columns, the node columns and types [0, 48), every further one the
 * next 48 types alone, its tables being the full tables advanced by 48 k entries.  The calls write disjoint outputs, so no
 * order between them matters; a call whose types are all empty launches nothing.  (data/graph_dataset.py assemble_batch.)
 * The node column fields were appended behind bad_flag: no earlier field moved, and struct_size tells a caller built against
 * the shorter struct apart.
 * ------------------------------------------------------------------------------------------ */
#define TFGNN_BATCH_MAX_EDGE_TYPES 48
#define TFGNN_BATCH_MAX_COLUMNS 8
#define TFGNN_BATCH_MAX_NODE_COLUMNS 4
typedef struct tfgnn_batch_assemble_args {
  size_t struct_size;
  int num_edge_types;
  int num_columns;
  int64_t num_graphs;  /* N */
  int64_t store_nodes; /* node_ptr[N] */
  int64_t feature_dim; /* F */
  /* fold store */
  const int32_t* node_ptr;
  const float* features;
  const int32_t* const* edge_ptr;
  const int32_t* const* edges;
  const float* const* columns;
  /* epoch */
  int64_t order_len; /* P */
  const int32_t* order;
  const int32_t* pos_node_ptr;
  const int32_t* const* pos_edge_ptr;
  /* batch */
  int64_t p0, p1;
  int64_t num_nodes;        /* V */
  const int64_t* num_edges; /* E_t */
  float* node_features;     /* [V, F] contiguous */
  int32_t* node_to_graph_map;
  int32_t* const* adjacency_lists; /* [E_t, 2] each */
  float* const* column_out;        /* [G] each */
  int* bad_flag;
  /* per-node columns */
  int num_node_columns;
  const int64_t* node_column_widths; /* W_c */
  const float* const* node_columns;  /* store [store_nodes, W_c] each */
  float* const* node_column_out;     /* [V, W_c] contiguous each */
} tfgnn_batch_assemble_args;
int tfgnn_batch_assemble(const tfgnn_batch_assemble_args* args, void* stream);
/* host-side count of the kernel launches tfgnn_batch_assemble has enqueued in this process: out[0]; further slots are zero */
int tfgnn_batch_assemble_launch_counts(int64_t* out_counts, int n);

/* ------------------------------------------------------------------------------------------
 * Neighbour sampling (csrc/sample.hip): a batch of seed nodes of ONE big graph -> one sampled K-hop subgraph, an ordinary
 * batch.  The reference has no such thing (its graphs are small); this is the GraphSAGE route for transductive tasks.
 *
 * Store (plain device arrays the caller owns; V = num_nodes < 2^31; built once per fold):
 *   per processed edge type t:  in_ptr[t] int32 [V + 1], in_src[t] int32 [E_t]: the sources of the in-edges of node v of
 *                               type t are in_src[t][in_ptr[t][v] .. in_ptr[t][v + 1]), in the fold's edge-list order (a
 *                               stable sort of the list by target).  store_edges[t] = E_t; sum_t E_t < 2^31.
 * One subgraph serves all K layers (the GNN runs every layer on the same adjacency lists): the in-neighbourhood of a node
 * is drawn ONCE per call, when the node is a frontier node, and the draw is a pure function of (seed, v, t).
 *
 * Order (all of it fixed: tests/neighbor_sample_reference.py reproduces the outputs exactly):
 *   nodes[0:S] = seeds, in the given order (distinct, in [0, V): see the status bits).  Frontier 1 = the seeds.
 *   hop h = 1..K, fanout f = fanouts[h - 1]: for every frontier node v in `nodes` order and every type t, with d the
 *   in-degree of type t of v:  c = d if f < 0 or d <= f, else f  (f = 0: no edges).  Edge j < c of row (v, t) is
 *       (in_src[t][in_ptr[t][v] + p_j], v)
 *   at position (edges of type t of earlier hops) + (sum of c over frontier nodes before v) + j of adjacency_lists[t].
 *   The sources that are not in `nodes` yet are appended to it in INCREASING GLOBAL ID; they are frontier h + 1.  After
 *   hop K nothing more is sampled: nodes first reached at hop K have no in-edges in the subgraph.
 *   p_j = j when c = d.  Otherwise p_j = (pi(j) + off) mod d, where, with k the row key,
 *       pi   a bijection of [0, d): an 8-round balanced Feistel network on b bits, b the smallest even number
 *            >= max(2, bit_length(d - 1)), x = (l << b/2) | r, round i = 0..7: (l, r) <- (r, l ^ F_i(r)),
 *            F_i(r) = (lowbias32(r ^ (k + i * 0x9E3779B9)) >> 7) & (2^(b/2) - 1); applied again while the value is >= d
 *       off  = lowbias32(k ^ 0xA5A5A5A5) mod d
 *       k    = lowbias32(lowbias32(v ^ s0) + (t + 1) * 0x9E3779B9) ^ s1     (32-bit wrap-around arithmetic)
 *       s0, s1: the low and high word of splitmix64's output for `seed` (z = seed + 0x9E3779B97F4A7C15;
 *            z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31 - the step the
 *            dropout keys use); lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *   These are c distinct positions, each computed by one thread on its own.
 * Outputs: nodes (global ids), adjacency_lists[t] int32 [*, 2] rows (source, target) in LOCAL ids (positions in `nodes`),
 * and meta, int32 [TFGNN_SAMPLE_META_WORDS(L, K)], for ONE device-to-host copy:
 *   meta[TFGNN_SAMPLE_META_STATUS]      0, or an OR of the TFGNN_SAMPLE_* bits below
 *   meta[TFGNN_SAMPLE_META_NODES]       n, the number of nodes
 *   meta[TFGNN_SAMPLE_META_EDGES + t]   the number of edges of type t
 *   meta[TFGNN_SAMPLE_META_EDGES + L + h], h = 0..K+1: hop_ptr - nodes[hop_ptr[h] : hop_ptr[h + 1]] were first reached at hop h
 *                                       (h = 0: the seeds), hop_ptr[K + 1] = n
 * Capacities: nothing is written at or beyond nodes[node_capacity] or row edge_capacity[t] of adjacency_lists[t].  What does
 * not fit is dropped and sets an overflow bit; the counts then stop at the capacities and the rest of the outputs is
 * unspecified (but written inside the capacities).  S <= node_capacity <= V.  A row is drawn once per call, so V nodes
 * and E_t edges always suffice; ops.sample_capacities gives the tighter bound from S, the fanouts and the largest in-degrees.
 * Status bits: a repeated seed (its rows are drawn more than once), a seed outside [0, V) (it has no in-edges), store
 * arrays that disagree with their sizes (the element is skipped or written as -1).
 *
 * Workspace: tfgnn_neighbor_sample_workspace_bytes(V, L, node_capacity) bytes, 16-byte aligned (0: arguments outside the
 * limits above).  Its first V int32 words are the local-id table: ALL -1 ON ENTRY - the caller fills it once, when it
 * allocates - and LEFT ALL -1 ON EXIT, by a pass over `nodes` (no memset of V), so calls follow one another on one
 * workspace.  The rest needs no initialisation.  A call that overflowed restores the table as well.
 *
 * 3 + 6 K launches on `stream` per call, whatever the fanouts (seeds; per hop: count, scan of the chunk totals, edge slots,
 * count of the marked ids, scan of those, assignment; translate; restore), every grid sized from the capacities: the sizes
 * exist on the device only.  No allocation, no copy, no synchronisation.  Parallel over output edge slots, a row found by
 * binary search in the scanned counts: a hub of thousands of in-edges is not one wave's loop.  "New nodes in increasing id"
 * is a scan over the table, where the slot pass marked them by plain stores of one value.  No float atomics; the only
 * atomic is an OR into the status word.
 * The pointer tables (in_ptr, in_src, store_edges, edge_capacity, adjacency_lists) and fanouts are HOST arrays read during
 * the call.
 * Rejected on the host before any HIP call: NULL args, another struct_size, num_hops outside [1, TFGNN_SAMPLE_MAX_HOPS],
 * num_seeds < 1, num_nodes < 1 or >= 2^31, negative sizes or capacities, sum_t E_t >= 2^31, a node capacity below S or
 * above V, NULL pointers, edge lists that are not 8-byte aligned, a workspace too small or unaligned.  More than
 * TFGNN_BATCH_MAX_EDGE_TYPES types: TFGNN_ERR_UNSUPPORTED.
 *
 * tfgnn_gather_node_rows: the rows of a sampled batch, ONE launch (none for num_rows == 0):
 *   node_features[i, :] = features[nodes[i], :],  node_column_out[c][i, :] = node_columns[c][nodes[i], :]   for i < num_rows,
 *   except that a column with seed_only[c] != 0 gets zeros in the rows i >= num_seeds.
 * The rules of tfgnn_batch_assemble: consecutive lanes on consecutive floats, per array float4 when its width % 4 == 0 and
 * both of its buffers are 16-byte aligned, rows_per_tile = clamp(8192 / width, 1, 256) rows to a workgroup, 64-bit element
 * offsets into the store.  A node id outside [0, store_nodes) skips its row and sets *bad_flag (nullable, zeroed by the
 * caller).  Nothing is written beyond num_rows rows.  Rejected on the host before any HIP call: NULL args, another
 * struct_size, negative sizes, store_nodes or num_rows >= 2^31, widths outside [1, 2^31), NULL pointers where num_rows > 0,
 * a NULL table when there are node columns.  More than TFGNN_BATCH_MAX_NODE_COLUMNS node columns: TFGNN_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
#define TFGNN_SAMPLE_MAX_HOPS 8
#define TFGNN_SAMPLE_META_STATUS 0
#define TFGNN_SAMPLE_META_NODES 1
#define TFGNN_SAMPLE_META_EDGES 2
#define TFGNN_SAMPLE_META_WORDS(L, K) (2 + (L) + (K) + 2)
#define TFGNN_SAMPLE_NODE_OVERFLOW 1
#define TFGNN_SAMPLE_EDGE_OVERFLOW 2
#define TFGNN_SAMPLE_REPEATED_SEED 4
#define TFGNN_SAMPLE_BAD_SEED 8
#define TFGNN_SAMPLE_BAD_STORE 16
typedef struct tfgnn_neighbor_sample_args {
  size_t struct_size;
  int num_edge_types; /* L */
  int num_hops;       /* K */
  int64_t num_nodes;  /* V */
  /* store */
  const int32_t* const* in_ptr;
  const int32_t* const* in_src;
  const int64_t* store_edges; /* E_t */
  /* call */
  const int32_t* fanouts; /* [K], < 0: every in-edge */
  uint64_t seed;
  int64_t num_seeds;    /* S */
  const int32_t* seeds; /* device [S] */
  /* outputs */
  int64_t node_capacity;
  const int64_t* edge_capacity;    /* [L] */
  int32_t* nodes;                  /* device [node_capacity] */
  int32_t* const* adjacency_lists; /* device [edge_capacity[t], 2] each */
  int32_t* meta;                   /* device [TFGNN_SAMPLE_META_WORDS(L, K)] */
  void* workspace;
  size_t workspace_bytes;
} tfgnn_neighbor_sample_args;
size_t tfgnn_neighbor_sample_workspace_bytes(int64_t num_nodes, int num_edge_types, int64_t node_capacity);
int tfgnn_neighbor_sample(const tfgnn_neighbor_sample_args* args, void* stream);

typedef struct tfgnn_gather_node_rows_args {
  size_t struct_size;
  int64_t store_nodes;  /* rows of `features` and of every node column */
  int64_t num_rows;     /* n */
  int64_t num_seeds;    /* S: the rows a seed_only column keeps */
  const int32_t* nodes; /* device [n], global ids */
  int64_t feature_dim;  /* F */
  const float* features;
  float* node_features; /* [n, F] contiguous */
  int num_node_columns;
  const int64_t* node_column_widths; /* W_c */
  const float* const* node_columns;  /* store [store_nodes, W_c] each */
  float* const* node_column_out;     /* [n, W_c] contiguous each */
  const int32_t* seed_only;          /* host [num_node_columns] */
  int* bad_flag;
} tfgnn_gather_node_rows_args;
int tfgnn_gather_node_rows(const tfgnn_gather_node_rows_args* args, void* stream);
/* host-side counts of the kernel launches enqueued in this process: out[0] by tfgnn_neighbor_sample (3 + 6 K per call),
 * out[1] by tfgnn_gather_node_rows (1 per call with rows); further slots are zero */
int tfgnn_sample_launch_counts(int64_t* out_counts, int n);

/* ------------------------------------------------------------------------------------------
 * Triple batches (csrc/triple_batch.hip): one mini-batch of link-prediction triples, built on the device.  A chunk of a
 * fold's positives plus fresh negatives becomes (a) the triples in global ids, (b) the DISTINCT endpoints in increasing
 * id - the seed list tfgnn_neighbor_sample demands - and (c) the triples in the batch's local ids.  The sampler puts its
 * seeds in rows 0 .. S - 1 of the sampled batch in the given order, so the rank of an endpoint in `seeds` IS its row in
 * the sampled batch: local_triples index the model's output directly.
 *
 * Inputs: V = num_nodes; positives int32 [P, 3], rows (u, t, v) in global ids (the fold's positives, uploaded once);
 * positive_ids int32 [B], the rows of this batch, in order (repeats allowed); K = negatives_per_positive >= 0; seed.
 * Outputs (device int32), N = B (1 + K):
 *   triples [N, 3]        rows 0 .. B - 1: triples[i] = positives[positive_ids[i]].  Rows B .. N - 1: exactly what
 *                         tfgnn_triples_draw_negatives(seed, use_epoch = 0) writes for these B positives: negative j copies
 *                         positive j / K of the batch and uses word(2 j), word(2 j + 1), the slot rule and the multiply-high
 *                         draw that skips the old node ("Negative sampling and triple tables on the device" above).  A
 *                         negative reads its positive from the store, not from this buffer.
 *   seeds [seed_capacity] seeds[0 : S] = the distinct endpoints (u and v of all N rows) in increasing global id.
 *   local_triples [N, 3]  (rank(u), t, rank(v)), rank = the position in `seeds`; the relation is copied.
 *   meta [2]              {status, S}, for ONE device-to-host copy (the sampler needs S on the host).
 * All of it is fixed, integers only: tests/triple_batch_reference.py restates every output bit for bit.
 * Status bits:
 *   TFGNN_TRIPLE_BATCH_SEED_OVERFLOW    more than seed_capacity distinct endpoints: S stops at the capacity, seeds holds the
 *                                       seed_capacity smallest, an endpoint beyond them gets local id -1, and nothing is
 *                                       written at or beyond a capacity.  min(2 N, V) always suffices.
 *   TFGNN_TRIPLE_BATCH_BAD_POSITIVE_ID  a positive_ids entry outside [0, P): its row - and the rows of its negatives - are
 *                                       (-1, -1, -1) in triples and in local_triples and contribute no seed.
 *   TFGNN_TRIPLE_BATCH_BAD_ENDPOINT     an endpoint outside [0, V): triples keeps the value, it contributes no seed and its
 *                                       local id is -1.
 * Every access of the store and of the table goes through an index checked against its size.
 *
 * Workspace: tfgnn_triple_batch_workspace_bytes(V) bytes, 16-byte aligned (0 for V outside [1, 2^31)).  Its first V int32
 * words are an id table under the sampler's convention: ALL -1 ON ENTRY - filled once by the caller - and LEFT ALL -1 ON
 * EXIT, in every case, overflow included; the rest needs no initialisation.  A sampler workspace of at least this size
 * serves (the sampler's table is its first V words, too).
 *
 * Exactly 6 launches on `stream`, whatever the sizes: (1) gather + draw + mark - the rows are written and
 * table[endpoint] = a marker where it was -1, plain stores of one value, idempotent; (2) marked ids per chunk of 1024 ids;
 * (3) ONE workgroup: scan of the chunk counts with a carry across rounds of 256 chunks, S, the overflow bit; (4) assign: a
 * marked id takes its rank, seeds[rank] = id, table[id] = rank; (5) translate; (6) restore.  Grids are sized from B, K, V
 * and the capacity; S exists on the device only.  No allocation, no copy, no host synchronisation, no float arithmetic; the
 * only atomic is an OR into the status word.
 * Refused on the host before any launch: NULL args or another struct_size; B < 1; K < 0; N > 2^30; P outside [1, 2^31);
 * V outside [1, 2^31); V < 2 with K > 0; seed_capacity < 1; NULL pointers; a short or misaligned workspace.
 *
 * tfgnn_triple_batch_launch_counts: out[0] = kernel launches enqueued by tfgnn_triple_batch_build in this process (6 per
 * call; a host counter); further slots are zero.
 * ------------------------------------------------------------------------------------------ */
#define TFGNN_TRIPLE_BATCH_SEED_OVERFLOW 1
#define TFGNN_TRIPLE_BATCH_BAD_POSITIVE_ID 2
#define TFGNN_TRIPLE_BATCH_BAD_ENDPOINT 4
typedef struct tfgnn_triple_batch_args {
  size_t struct_size;
  int64_t num_nodes;              /* V */
  int64_t num_positives;          /* P */
  const int32_t* positives;       /* device [P, 3] */
  int64_t batch_size;             /* B */
  const int32_t* positive_ids;    /* device [B] */
  int64_t negatives_per_positive; /* K */
  uint64_t seed;
  int64_t seed_capacity;
  /* outputs */
  int32_t* triples;       /* device [N, 3] */
  int32_t* local_triples; /* device [N, 3] */
  int32_t* seeds;         /* device [seed_capacity] */
  int32_t* meta;          /* device [2] */
  void* workspace;
  size_t workspace_bytes;
} tfgnn_triple_batch_args;
size_t tfgnn_triple_batch_workspace_bytes(int64_t num_nodes);
int tfgnn_triple_batch_build(const tfgnn_triple_batch_args* args, void* stream);
int tfgnn_triple_batch_launch_counts(int64_t* out_counts, int n);

/* ------------------------------------------------------------------------------------------
 * Excluding a batch's positives (csrc/sample_exclude.hip): the edges whose score a link-prediction mini-batch trains are
 * taken out of the subgraph the sampler drew for it.  Both endpoints of a positive (u, r, v) are seeds, so the sampler
 * draws row (v, type of r) at hop 1 and - at fanout -1 always - hands the encoder the very edge u -> v, and v -> u on the
 * inverse type.  tfgnn_sample_exclude_edges runs on the outputs of tfgnn_neighbor_sample, on the same stream, BEFORE the
 * sampler's meta words are copied to the host: draw first, then drop.
 *
 * Inputs: L = num_edge_types lists adjacency_lists[t] int32 [edge_capacity[t], 2] in LOCAL ids (after the sampler's
 * translate pass) with their live counts in meta[TFGNN_SAMPLE_META_EDGES + t]; S = num_seeds; positives int32 [B, 3], rows
 * (u, r, v) in local ids - rows 0 .. B - 1 of tfgnn_triple_batch_build's local_triples; and two HOST tables over the
 * T = num_relations relations, read during the call: fwd_type[r], the processed edge type that carries the forward edges
 * of relation r, and inv_type[r], the type that carries their inverses (the same type for a tied relation, the backward
 * type otherwise); -1 = none.
 * For every positive (u, r, v) the call removes from list fwd_type[r] every edge (u, v) and from list inv_type[r] every
 * edge (v, u) - multi-edges all go, a repeated positive removes nothing more, u == v on a tied type removes the loops
 * (u, u) of that list.  Types that no table entry names (the self loops) are never touched.
 * PRECONDITION the sampler guarantees: every list is sorted by target (hops append rows in frontier order and frontier
 * local ids increase).  Both endpoints are seeds and a row is drawn once, when its node is a frontier node, so every
 * such edge sits in a hop-1 row and its endpoints are in `nodes` regardless: nodes, hop_ptr and the node count do not
 * change, and dropping after the whole sample equals dropping per hop.  At a finite fanout a row may keep fewer than f
 * edges: nothing is drawn in place of a dropped edge.
 *
 * Outputs:
 *   adjacency_lists[t][0 : new count)   the kept edges in their old order.  Nothing is written at or beyond the OLD
 *                                       count; the slots between the new and the old count are unspecified.
 *   meta[TFGNN_SAMPLE_META_EDGES + t]   the new count, in place: the sampler's one device-to-host copy carries it.
 *   meta[TFGNN_SAMPLE_META_STATUS]      OR-ed with the status word below (the bits do not collide with TFGNN_SAMPLE_*).
 *   record int32 [TFGNN_SAMPLE_EXCLUDE_RECORD_WORDS(L)]:  record[t] = removed[t] = old count - new count, record[L] =
 *                                       the status word: 0 or an OR of
 *       TFGNN_SAMPLE_EXCLUDE_BAD_RELATION   a positive whose relation is outside [0, T)
 *       TFGNN_SAMPLE_EXCLUDE_BAD_ENDPOINT   a positive with an endpoint outside [0, S)
 *                                       Such a row is skipped.  A row (-1, -1, -1) - what tfgnn_triple_batch_build writes
 *                                       for a bad positive id - is skipped and sets no bit.
 * An edge whose source is -1 (the sampler's mark of a bad store entry) is kept.  A live count above its capacity is read
 * as the capacity.  All of it is fixed, integers only: tests/sample_exclude_reference.py restates it.
 *
 * Workspace: tfgnn_sample_exclude_workspace_bytes(L, edge_capacity) bytes, 16-byte aligned (0 for arguments outside the
 * limits below); no initialisation.  It holds a packed copy of the lists (sum_t ceil(cap_t / 1024) * 1024 edges).
 *
 * Exactly TFGNN_SAMPLE_EXCLUDE_LAUNCHES = 4 launches on `stream`, whatever the sizes: (1) mark - one wave per
 * (positive, direction): a binary search for the target's row, then the wave strides over the row and overwrites the
 * source of every matching edge with a marker, plain stores of one value, idempotent; a hub row with hundreds of
 * positives pointing at it is hundreds of strided walks, not one thread's loop; (2) pack - per chunk of 1024 slots, the
 * types flattened into one grid: the unmarked edges, in order, into the workspace, and their number; (3) ONE workgroup:
 * scan of the chunk counts with a carry across rounds of 256 chunks, the new counts, removed[], the status; (4) move
 * - the packed chunks back into the lists at their scanned offsets.  Grids are sized from B and the capacities; the live
 * counts exist on the device only.  No allocation, no copy, no host synchronisation, no float arithmetic; the only
 * atomic is an OR into the status word.  The per-type pointers and both tables travel as kernel arguments.
 * Refused on the host before any HIP call: NULL args or another struct_size; negative sizes or capacities; B < 1 or
 * > 2^30; S >= 2^31; a capacity >= 2^31 or 2^31 or more slots in all; a table entry outside [-1, L); NULL pointers;
 * edge lists that are not 8-byte aligned; a short or misaligned workspace.  More than TFGNN_BATCH_MAX_EDGE_TYPES types
 * or relations: TFGNN_ERR_UNSUPPORTED.
 *
 * tfgnn_sample_exclude_launch_counts: out[0] = kernel launches enqueued by tfgnn_sample_exclude_edges in this process
 * (4 per call; a host counter); further slots are zero.
 * ------------------------------------------------------------------------------------------ */
#define TFGNN_SAMPLE_EXCLUDE_LAUNCHES 4
#define TFGNN_SAMPLE_EXCLUDE_BAD_RELATION 32
#define TFGNN_SAMPLE_EXCLUDE_BAD_ENDPOINT 64
#define TFGNN_SAMPLE_EXCLUDE_RECORD_WORDS(L) ((L) + 1)
typedef struct tfgnn_sample_exclude_args {
  size_t struct_size;
  int num_edge_types;              /* L */
  int num_relations;               /* T */
  int64_t num_seeds;               /* S */
  int64_t num_positives;           /* B */
  const int32_t* positives;        /* device [B, 3], local ids */
  const int32_t* fwd_type;         /* host [T] */
  const int32_t* inv_type;         /* host [T] */
  const int64_t* edge_capacity;    /* host [L] */
  int32_t* const* adjacency_lists; /* host [L] of device [edge_capacity[t], 2] */
  int32_t* meta;                   /* device: the sampler's meta words */
  int32_t* record;                 /* device [TFGNN_SAMPLE_EXCLUDE_RECORD_WORDS(L)] */
  void* workspace;
  size_t workspace_bytes;
} tfgnn_sample_exclude_args;
size_t tfgnn_sample_exclude_workspace_bytes(int num_edge_types, const int64_t* edge_capacity);
int tfgnn_sample_exclude_edges(const tfgnn_sample_exclude_args* args, void* stream);
int tfgnn_sample_exclude_launch_counts(int64_t* out_counts, int n);

/* ------------------------------------------------------------------------------------------
 * R-GCN basis decomposition (csrc/basis.hip; Schlichtkrull et al. 2018, eq. 3: W_l = sum_b a[l,b] V_b with B shared bases),
 * aggregate first.  With s_e / m_v the scales of tfgnn_graph_scales (d_edge_weight_by_dst / d_node_scale), L the handle's
 * number of edge types and coeff = a [L, B] contiguous:
 *   tfgnn_basis_gather_forward   Z[v, b*D + d] = m_v * sum over the edges e = (u -> v) of type l of  s_e * a[l,b] * X[u, d]
 *   tfgnn_basis_gather_backward  dX[u, d]     = sum over the edges e = (u -> v) of type l of  s'_e * sum_b a[l,b] * dZ[v, b*D + d]
 *                                               (s' = d_edge_weight_by_src, which carries m_v)
 *                                dcoeff[l, b] = sum over the nodes v of  m_v * < dZ[v, b*D .. b*D + D), S[v, l, :] >,
 *                                               S[v, l, :] = sum over the edges e = (u -> v) of type l of  s_e * X[u, :]
 *                                               - recomputed from X, never stored (it is the [V, L*D] operand of the plain layer)
 * Z feeds one product with the stacked bases [B*D, H] (tfgnn_gemm and friends); the gather writes B*D floats per node instead
 * of L*D.  X, Z, dZ, dX have row strides (floats); columns outside [0, B*D) / [0, D) of a wider array are left untouched.
 * edge_weight_* NULL: 1 per edge; node_scale NULL: 1.  dX / dcoeff NULL: not computed.
 *
 * The walks use the handle's node views (TFGNN_G_NODEPTR_BY_DST + TFGNN_G_COLL_BY_DST, ..._BY_SRC: other end = coll / L,
 * type = coll % L; inside a node's row the edges are sorted by type) and their long-row plans (part PLAN_NODE): a row of more
 * than 32 edges is cut into items of 512 edges, one workgroup per item, whose G lane groups (G = 16, 8 or 4 for rows of at
 * most 64 (16 on the scalar path), at most 128, or more floats) take ceil(edges / G) consecutive edges each.  A row of at most
 * 32 edges is one segment.  ORDER OF THE SUMS - fp32, fused multiply-adds, no float atomics; it depends on the graph (and on
 * B, D, the alignment) alone, so two calls - or an eager call and its replay from a captured graph - give the same bits:
 *   forward  per segment: the edges in by-target order; inside a run of one type  r = fma(s_e, x, r);  at the end of a run
 *            acc_b = fma(a[l,b], r, acc_b), runs in ascending type.  The segments of an item are added in order, the items of
 *            a row in item order (second launch, only when some row has several items), then * m_v.
 *   dX       per segment: the edges in by-source order;  t = sum_b fma(a[l,b], dz, t) with b ascending;  acc = fma(s'_e, t, acc).
 *            Segments and items as above.
 *   dcoeff   per run of one type inside a segment: r as in forward; per lane  p_b = fma(r, dz, p_b)  over the lane's columns
 *            ascending; the lanes of the group by a butterfly (xor 32/16/8 .. 1); * m_v.  The run's B numbers are stored at the
 *            run's first edge in a zeroed [E, B] table.  Stage 1: workgroup (chunk c of 1024 nodes, type l), wave w adds the table
 *            rows of the edges of type l into v = 1024 c + w, + 4, ... in edge order, then ((w0 + w1) + w2) + w3.  Stage 2:
 *            dcoeff[l, b] = the chunk sums in chunk order.  Partial tables plus an ordered reduce: needs no COMPACT part.
 * The vector path (16-byte loads) is taken when D % 4 == 0 and the rows involved are 16-byte aligned (base and stride), the
 * scalar path otherwise.  Neither counts arrivals nor waits on other workgroups, so the concurrency caveat of the
 * tfgnn_graph_gather_* functions does not apply: calls over one handle may be in flight on several streams as long as
 * each has a workspace of its own.
 *
 * Launches per call: forward 1 (+ 1 when a target row has several items); backward: dX 1 (+ 1), dcoeff 3 and one memset.  No
 * allocation, no synchronisation, nothing read back: capturable as they are.
 * workspace: tfgnn_basis_workspace_bytes(V, E, L, B, D, partials_by_dst, partials_by_src) bytes, 16-byte aligned, where
 * partials_* = tfgnn_graph_gather_workspace_bytes(graph, TFGNN_VIEW_BY_DST_NODE / _BY_SRC_NODE, 1) / 4 (the plans' item counts
 * of multi-item rows); one size serves both calls (0 for values outside the limits).
 * LIMITS, checked on the host before the first launch: a struct of another size, NULL graph / pointers, strides smaller than
 * the rows, a handle without PLAN_NODE, num_bases < 1, D < 1: TFGNN_ERR_INVALID_ARGUMENT; num_bases > 64, D > 2^20,
 * B * D >= 2^31: TFGNN_ERR_UNSUPPORTED or INVALID_ARGUMENT with a message that names the limit.  L is the handle's (<= 256).
 * V == 0: nothing launched.  No edges, an edge type without edges, a node without in- / out-edges: zeros (dcoeff[l, :] = 0).
 * ------------------------------------------------------------------------------------------ */
typedef struct tfgnn_basis_forward_args {
  size_t struct_size;
  const tfgnn_graph* graph;
  int B, D;                        /* num_bases, input width */
  const float* coeff;              /* [L, B] */
  const float* X;                  /* [V, D], row stride ldX */
  int64_t ldX;
  const float* edge_weight_by_dst; /* [E] or NULL */
  const float* node_scale;         /* [V] or NULL */
  float* Z;                        /* [V, B*D], row stride ldZ */
  int64_t ldZ;
  void* workspace;
  size_t workspace_bytes;
} tfgnn_basis_forward_args;

typedef struct tfgnn_basis_backward_args {
  size_t struct_size;
  const tfgnn_graph* graph;
  int B, D;
  const float* coeff;              /* [L, B] */
  const float* dZ;                 /* [V, B*D], row stride lddZ */
  int64_t lddZ;
  const float* X;                  /* [V, D], row stride ldX; read for dcoeff only (may be NULL without it) */
  int64_t ldX;
  const float* edge_weight_by_dst; /* [E] or NULL: dcoeff */
  const float* edge_weight_by_src; /* [E] or NULL: dX */
  const float* node_scale;         /* [V] or NULL: dcoeff */
  float* dX;                       /* [V, D], row stride lddX; NULL = not wanted */
  int64_t lddX;
  float* dcoeff;                   /* [L, B] contiguous; NULL = not wanted */
  void* workspace;
  size_t workspace_bytes;
} tfgnn_basis_backward_args;

size_t tfgnn_basis_workspace_bytes(int64_t V, int64_t E, int L, int B, int D, int64_t partials_by_dst, int64_t partials_by_src);
int tfgnn_basis_gather_forward(const tfgnn_basis_forward_args* args, void* stream);
int tfgnn_basis_gather_backward(const tfgnn_basis_backward_args* args, void* stream);
/* host-side counts of the kernel launches enqueued in this process: out[0] forward gather ("basis_fwd"), out[1] dX
 * ("basis_dx"), out[2] dcoeff ("basis_dcoeff"), combining / reducing launches included; further slots are zero */
int tfgnn_basis_launch_counts(int64_t* out_counts, int n);

/* ------------------------------------------------------------------------------------------
 * R-GCN block-diagonal decomposition (csrc/blockdiag.hip; Schlichtkrull et al. 2018, eq. 4: W_l = blockdiag(Q_l^0 .. Q_l^{C-1})
 * with C = num_blocks blocks Q_l^c [di, ho], di = D / C, ho = H / C, both exact), the blocks applied inside the neighbour walk.
 * The blocks are stored BANDED in one contiguous buffer Qb [L, di, H]:
 *   W_l[c*di + i, c*ho + j] = Qb[l, i, c*ho + j]          (every other entry of W_l is 0)
 * so output column h reads Qb[l, i, h], i = 0 .. di-1: rows of H floats.  With s_e / m_v / s'_e the scales of tfgnn_graph_scales
 * (d_edge_weight_by_dst / d_node_scale / d_edge_weight_by_src, which carries m_v), c(h) = h / ho and c(d) = d / di:
 *   tfgnn_blockdiag_forward   pre[v, h]    = m_v * sum over the edges e = (u -> v) of type l of
 *                                            s_e * sum_i X[u, c(h)*di + i] * Qb[l, i, h]
 *   tfgnn_blockdiag_backward  dX[u, d]     = sum over the edges e = (u -> v) of type l of
 *                                            s'_e * sum_j dPre[v, c(d)*ho + j] * Qb[l, d % di, c(d)*ho + j]
 *                             dQb[l, i, h] = sum over the edges e = (u -> v) of type l of  m_v * s_e * X[u, c(h)*di + i] * dPre[v, h]
 * pre is the layer's output before its activation (tfgnn_activation_forward / _backward stay separate passes).  No per-bucket
 * operand, no per-edge message and no product: Qb (L * D * H / C floats) is read through the caches.  X, pre, dPre, dX have row
 * strides (floats); columns outside [0, D) / [0, H) of a wider array are left untouched.  edge_weight_* NULL: 1 per edge;
 * node_scale NULL: 1.  dX / dQb NULL: not computed; each alone gives the same bits as both together.
 *
 * The two walks use the handle's node views and their long-row plans (part PLAN_NODE) exactly as the basis gather above: a row
 * of more than 32 edges is cut into items of 512 edges, one workgroup per item, whose G lane groups take ceil(edges / G)
 * consecutive edges each; a row of at most 32 edges is one segment.  A lane group of P lanes owns a WINDOW of cw whole blocks on
 * both sides (their cw*di input and cw*ho output columns; blockIdx.y walks the ceil(C / cw) windows): with u = 4 on the vector
 * path and 1 on the scalar path, P is the one of 16, 32, 64 with cw = min(C, floor(P*u / max(di, ho))) >= 1 for which
 * ceil(C / cw) * P is smallest (ties: the larger P), and G = 256 / P.
 * ORDER OF THE SUMS - fp32, fused multiply-adds, no float atomics; it depends on the graph, C, D, H and the alignment alone, so
 * two calls - or an eager call and its replay from a captured graph - give the same bits:
 *   forward  per segment: the edges in by-target order; inside a run of one type  r[d] = fma(s_e, x[d], r[d]);  at the end of
 *            the run, once per run,  acc[h] = fma(r[c(h)*di + i], Qb[l, i, h], acc[h])  with i ascending; runs in ascending
 *            type.  The segments of an item are added in order, the items of a row in item order (second launch, only when
 *            some row has several items), then * m_v.
 *   dX       per segment: the edges in by-source order; inside a run  g[h] = fma(s'_e, dPre[v, h], g[h]);  at the end of the run
 *            acc[d] = fma(g[c(d)*ho + j], Qb[l, d % di, c(d)*ho + j], acc[d])  with j ascending.  Segments and items as above.
 *   dQb      type-major, two stages.  The concatenation of the caller's edge lists is type-major; chunk k of type l is its list
 *            positions [first_l + 256 k, first_l + min(E_l, 256 (k + 1))).  Stage 1, one workgroup per chunk (and tile of 64
 *            columns x 8 block rows): wave w of 4 takes the w-th run of ceil(n / 4) consecutive positions of the chunk's n;
 *            per edge  t = (m_v * s_e) * dPre[v, h]  (two roundings) and  p[i] = fma(X[u, c(h)*di + i], t, p[i]);  the four
 *            waves' sums as ((w0 + w1) + w2) + w3.  Stage 2: dQb[l, i, h] = 0 + the chunk partials of type l in chunk order;
 *            a type without edges gets exact zeros.
 * The vector path (16-byte loads) is taken when di % 4 == 0, ho % 4 == 0 and the rows involved are 16-byte aligned (base and
 * stride; forward: X, pre and Qb; dX: dPre and dX), the scalar path otherwise.  Nobody counts arrivals or waits on another
 * workgroup: calls over one handle may be in flight on several streams as long as each has a workspace of its own.
 *
 * dQb reads four int32 device tables that the caller builds once per graph (ops.py keeps them with the Graph): list_to_dst [E],
 * the inverse of TFGNN_G_EID_BY_DST (position in the concatenated lists -> position in the by-target order); chunk_first and
 * chunk_count [num_chunks], the first list position and the length (1 .. 256) of every chunk, types ascending, chunks of a type
 * ascending; type_chunk_ptr [L + 1], the first chunk of every type.  num_chunks = sum_l ceil(E_l / 256).  The tables are trusted.
 *
 * Launches per call: forward 1 (+ 1 when a target row has several items); backward: dX 1 (+ 1), dQb 2 (without edges: one
 * memset instead).  No allocation, no synchronisation, nothing read back: capturable as they are.
 * workspace: tfgnn_blockdiag_workspace_bytes(C, D, H, partials_by_dst, partials_by_src, num_chunks) bytes, 16-byte aligned:
 * max(partials_by_dst * H, partials_by_src * D + num_chunks * di * H) floats (each part rounded up to 16 bytes), partials_* as
 * for the basis gather; one size serves both calls (0 for values outside the limits).
 * LIMITS, checked on the host before the first launch: a struct of another size, NULL graph / pointers, strides smaller than
 * the rows, a handle without PLAN_NODE, num_blocks < 1, D or H < 1, num_blocks not dividing D and H:
 * TFGNN_ERR_INVALID_ARGUMENT; a block wider than the lane mapping holds - D / num_blocks > 64 or H / num_blocks > 64 (D and H
 * themselves are not capped) - or num_blocks > 65535: TFGNN_ERR_UNSUPPORTED; each with a message that names the limit.
 * V == 0: nothing launched.  No edges, an edge type without edges, a node without in- / out-edges: zeros.
 * ------------------------------------------------------------------------------------------ */
typedef struct tfgnn_blockdiag_forward_args {
  size_t struct_size;
  const tfgnn_graph* graph;
  int C, D, H;                     /* num_blocks, input width, output width */
  const float* Qb;                 /* [L, D/C, H] contiguous */
  const float* X;                  /* [V, D], row stride ldX */
  int64_t ldX;
  const float* edge_weight_by_dst; /* [E] or NULL */
  const float* node_scale;         /* [V] or NULL */
  float* pre;                      /* [V, H], row stride ldpre */
  int64_t ldpre;
  void* workspace;
  size_t workspace_bytes;
} tfgnn_blockdiag_forward_args;

typedef struct tfgnn_blockdiag_backward_args {
  size_t struct_size;
  const tfgnn_graph* graph;
  int C, D, H;
  const float* Qb;                 /* [L, D/C, H] contiguous; read for dX only (may be NULL without it) */
  const float* dPre;               /* [V, H], row stride lddPre */
  int64_t lddPre;
  const float* X;                  /* [V, D], row stride ldX; read for dQb only (may be NULL without it) */
  int64_t ldX;
  const float* edge_weight_by_dst; /* [E] or NULL: dQb */
  const float* edge_weight_by_src; /* [E] or NULL: dX */
  const float* node_scale;         /* [V] or NULL: dQb */
  float* dX;                       /* [V, D], row stride lddX; NULL = not wanted */
  int64_t lddX;
  float* dQb;                      /* [L, D/C, H] contiguous; NULL = not wanted */
  const int32_t* list_to_dst;      /* [E]; the four tables are read for dQb only */
  const int32_t* chunk_first;      /* [num_chunks] */
  const int32_t* chunk_count;      /* [num_chunks] */
  const int32_t* type_chunk_ptr;   /* [L + 1] */
  int64_t num_chunks;
  void* workspace;
  size_t workspace_bytes;
} tfgnn_blockdiag_backward_args;

size_t tfgnn_blockdiag_workspace_bytes(int C, int D, int H, int64_t partials_by_dst, int64_t partials_by_src, int64_t num_chunks);
int tfgnn_blockdiag_forward(const tfgnn_blockdiag_forward_args* args, void* stream);
int tfgnn_blockdiag_backward(const tfgnn_blockdiag_backward_args* args, void* stream);
/* host-side counts of the kernel launches enqueued in this process: out[0] forward ("fwd"), out[1] dX ("dx"), out[2] dQb
 * ("dq"), combining / reducing launches included; further slots are zero */
int tfgnn_blockdiag_launch_counts(int64_t* out_counts, int n);

/* ------------------------------------------------------------------------------------------
 * Node embeddings (csrc/embedding.hip): the gradient of a row lookup with DISTINCT ids, written as a dense table gradient.
 * The lookup itself is tfgnn_gather_node_rows.
 *
 *   table_grad[r, 0:D] = rows[i, 0:D]   if ids[i] == r for some i < n
 *                      = 0              otherwise,                        for every r < N
 *
 * rows fp32 [n, D] with row pitch ld_rows, ids int32 [n], table_grad fp32 [N, D] with row pitch ld_grad (pitches in floats).
 * Columns >= D of a pitched row are not touched.  An id outside [0, N) skips its row and sets *bad_flag (nullable, zeroed by
 * the caller).  The ids are distinct by precondition - the neighbour sampler guarantees it (TFGNN_SAMPLE_REPEATED_SEED) -;
 * with a repeated id ONE of its rows is written, which one is unspecified, and nothing else is affected.
 *
 * At most two launches on `stream`: a fill of all N rows and a scatter of the n rows; one (the fill) for n == 0, none for
 * N == 0.  No allocation, no copy, no synchronisation, no atomics: capturable.  Consecutive lanes work on consecutive floats
 * of a row, the rule of tfgnn_batch_assemble: float4 when D % 4 == 0, both buffers are 16-byte aligned and both pitches are
 * multiples of 4; clamp(8192 / D, 1, 256) rows to a workgroup.  Element offsets are 64-bit: N * D may pass 2^31.
 * Rejected on the host before any HIP call: negative sizes, D < 1 or >= 2^31, a pitch below D, N >= 2^31, n > N, a NULL
 * table_grad when N > 0, NULL rows or ids when n > 0.
 * ------------------------------------------------------------------------------------------ */
int tfgnn_embedding_scatter_rows(const float* rows, int64_t ld_rows, const int32_t* ids, int64_t n, int64_t D,
                                 float* table_grad, int64_t ld_grad, int64_t N, int* bad_flag, void* stream);
/* host-side count of the kernel launches tfgnn_embedding_scatter_rows has enqueued in this process (tests) */
int64_t tfgnn_embedding_launch_count(void);

#ifdef __cplusplus
}
#endif
#endif /* TFGNN_H */
