/*
 * safe_hip.h -- C ABI of libsafe_hip.so: the MI355X (gfx950) implementation of the
 * SAFE hot path (neighborhood definition + enrichment p-values).
 *
 * The reference (baryshnikova-lab/safepy) is pure Python and has no FFI; this header
 * is the boundary a maintainer binds with ctypes.  Every entry
 * point cites the reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns 0 on success, a negative SAFE_E_* code on failure;
 *     safe_last_error() returns a thread-local message for the last failure.
 *   - "host" pointers are ordinary process memory owned by the caller; "dev" pointers
 *     are HIP device memory (from safe_dev_alloc or any other HIP allocator, e.g. a
 *     torch tensor's data_ptr()).  Outputs are always pre-allocated by the caller.
 *   - the library owns device memory only behind its opaque handles.
 *   - work is enqueued on the context's stream (safe_ctx_set_stream; default: a
 *     stream the context owns).  The library runs further streams of its own behind
 *     it; every call orders them after what is already queued on the context's stream
 *     and joins them back before it returns, so a caller orders their own work against
 *     the context's stream alone.  Functions with host outputs synchronise before
 *     returning.  Of the functions with only dev outputs these return WITHOUT waiting:
 *     safe_euclidean_dense_dev, safe_nbr_to_dense_i64_dev, safe_dev_memset,
 *     safe_attr_create_dev, safe_export_packed_counts, safe_export_packed_chunk(_narrow)
 *     and safe_outputs_from_packed_slabs (once its NES table is resident: from the
 *     second call with the same table on).  The others enqueue on the
 *     context's stream like them but return only once it has drained, because they read
 *     a flag or a timing event back or keep host memory alive for their kernels:
 *     safe_score, safe_permtest_counts, safe_randomization, safe_hypergeom,
 *     safe_hypergeom_tails, safe_hypergeom_outputs, safe_moments_test, safe_score_weighted, safe_moments_test_weighted,
 *     safe_permtest_counts_weighted, safe_permtest_extremes, safe_counts_from_extremes, safe_fdr_adjust, safe_fdr_adjust_rows,
 *     safe_fdr_adjust_scope, safe_fdr_adjust_matrix, safe_mt_adjust_scope, safe_mt_adjust_matrix,
 *     safe_outputs_from_counts, safe_outputs_from_packed_counts,
 *     safe_nes_from_packed_counts and safe_attr_nan_to_zero
 *     (tests/test_gpu_stream_order.py measures both lists).
 *   - safe_ctx_set_stream orders the stream it switches to behind the one it leaves:
 *     handles created, buffers borrowed and outputs written on the old stream are
 *     complete for everything enqueued afterwards.  The stream being left must still
 *     exist at that moment.
 *   - one context per device; a context is not thread-safe.
 *   - there is NO CPU fallback: without a HIP device every compute call fails.
 */
#ifndef SAFE_HIP_H
#define SAFE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAFE_HIP_ABI_VERSION 9

#define SAFE_OK 0
#define SAFE_E_INVALID (-1)   /* bad argument */
#define SAFE_E_HIP (-2)       /* HIP runtime error (message has the hipError string) */
#define SAFE_E_NOMEM (-3)
#define SAFE_E_UNSUPPORTED (-4)
#define SAFE_E_VALUE (-5)     /* input data violates a contract (e.g. non-0/1 membership) */

#define SAFE_DTYPE_F32 0
#define SAFE_DTYPE_F64 1
#define SAFE_DTYPE_U8 2       /* safe_attr_create_host only: 0/1 (or small integer) values as bytes, no missing values */

#define SAFE_SCORE_SUM 0      /* neighborhood_score_type == 'sum'     */
#define SAFE_SCORE_ZSCORE 1   /* neighborhood_score_type == 'z-score' */

#define SAFE_SIGN_HIGHEST 0   /* attribute_sign == 'highest' */
#define SAFE_SIGN_LOWEST 1    /* attribute_sign == 'lowest'  */
#define SAFE_SIGN_BOTH 2      /* attribute_sign == 'both'    */

#define SAFE_FDR_SCOPE_ROWS 0 /* multiple_testing_scope == 'attributes': every node's row (the reference)  */
#define SAFE_FDR_SCOPE_COLS 1 /* multiple_testing_scope == 'neighborhoods': every attribute's column       */
#define SAFE_FDR_SCOPE_ALL 2  /* multiple_testing_scope == 'all': the whole matrix as one family           */

typedef struct safe_ctx safe_ctx;
typedef struct safe_nbr safe_nbr;       /* neighborhood membership, device resident     */
typedef struct safe_attr safe_attr;     /* node x attribute matrix, device resident     */
typedef struct safe_perms safe_perms;   /* composed row-permutation tables, device res. */
typedef struct safe_comm safe_comm;     /* RCCL communicator of the attribute-sharded path */
typedef struct safe_kk safe_kk;         /* Kamada-Kawai cost function of one distance matrix, device res. */
typedef struct safe_pairs safe_pairs;   /* one selection of a result matrix, counted and scanned, device res. */
typedef struct safe_go safe_go;         /* propagated gene-to-term annotations as CSC, device resident */
typedef struct PermRing safe_ring;      /* node-shared permutation stream (shared memory)    */

/* ------------------------------------------------------------------ context ---- */
int safe_abi_version(void);
const char *safe_last_error(void);
int safe_device_count(int *count);
/* PCI address of a device ("0000:c1:00.0"): lets the host side keep a rank's threads on the NUMA node of its GPU
 * (safepy_amd.backend.pin_threads_to_device_numa; the reference has no counterpart -- its multiprocessing
 * workers, safe.py:503-524, run wherever the OS puts them). */
int safe_device_pci_bus_id(int device, char *buf, size_t buf_len);
int safe_ctx_create(int device, safe_ctx **out);
int safe_ctx_destroy(safe_ctx *ctx);
/* Host waits of every context in this process: 0 (default) = hipStreamSynchronize, the runtime spins (lowest latency, one
 * busy core per waiting thread); 1 = sleep on interrupt-backed events (several ranks sharing few host cores: the
 * reference's worker pool, safepy/safe.py:503-524, simply oversubscribes).  Set before the first context is created;
 * SAFE_HIP_BLOCKING_SYNC=1 in the environment has the same effect. */
int safe_set_blocking_sync(int on);
/* Use an existing hipStream_t (passed as void*) for all subsequent work; NULL restores
 * the context's own stream.  When the stream changes, an event is recorded on the old
 * stream and the new one waits for it (see Conventions). */
int safe_ctx_set_stream(safe_ctx *ctx, void *hip_stream);
int safe_ctx_sync(safe_ctx *ctx);
int safe_ctx_info(safe_ctx *ctx, int *num_cu, int64_t *hbm_bytes, char *arch, size_t arch_len);
/* How this library was built: the compiler version and the verdict of the build's disassembly check of the bit-sliced
 * permutation kernel's hidden registers (the kernel behind run_permutations, safepy/safe_extras.py:36-70, keeps two id quads in
 * registers the compiler does not allocate; a library built where the check could not run uses the form without them). */
int safe_build_info(char *out, size_t out_len);
int safe_dev_alloc(safe_ctx *ctx, size_t bytes, void **out_dev);
int safe_dev_free(safe_ctx *ctx, void *dev);
int safe_dev_memset(safe_ctx *ctx, void *dev, int value, size_t bytes);
int safe_memcpy_h2d(safe_ctx *ctx, void *dev, const void *host, size_t bytes);   /* synchronous */
int safe_memcpy_d2h(safe_ctx *ctx, void *host, const void *dev, size_t bytes);   /* synchronous */
/* The same copy for a destination whose pages are RESIDENT (an array that has been written before, e.g. the recycled host
 * array of a result matrix -- self.nes and its siblings, safepy/safe.py:530-554): one plain copy at the link's rate (56 GB/s
 * measured), no helper threads.  (safe_memcpy_d2h spreads the page faults of a FRESH destination over copy threads.) */
int safe_memcpy_d2h_resident(safe_ctx *ctx, void *host, const void *dev, size_t bytes);
/* Event pair on the context stream, for timing a region that runs on that stream. */
int safe_timer_start(safe_ctx *ctx);
int safe_timer_stop_ms(safe_ctx *ctx, double *elapsed_ms);   /* synchronises */

/* ------------------------------------------------------------ neighborhoods ---- */
/* Replaces SAFE.define_neighborhoods, 'euclidean' branch (safepy/safe.py:389-399):
 * A[i,j] = (sqrt(dx*dx + dy*dy) < nr), each op rounded to f64 (scipy pdist), diagonal
 * kept.  xy_host is [n,2] row-major; nr = radius * (max x - min x) is computed by the
 * caller exactly as safe.py:390-391 does. */
int safe_nbr_euclidean(safe_ctx *ctx, const double *xy_host, int64_t n, double nr, safe_nbr **out);

/* Replaces the two shortest-path branches (safepy/safe.py:401-417; networkx
 * all_pairs_dijkstra_path_length with cutoff): A[s,t] = 1 iff the shortest-path length
 * from s to t is <= cutoff.  Undirected edges (edge_u[e], edge_v[e]) with weight
 * edge_w[e] ('length' for shortpath_weighted_layout) or unit weight when edge_w is NULL
 * ('shortpath').  keep_distances != 0 also keeps the dense f64 distance matrix
 * (inf where unreached) for safe_nbr_distances (self.node_distances, safe.py:417).
 * Two edges between one pair of nodes are both kept, so the smaller weight wins; nx.Graph
 * would keep only the weight added last, and de-duplicating is the caller's job.
 * A negative, NaN or infinite weight is SAFE_E_INVALID: with cutoff = +inf networkx counts a
 * node behind a path of length +inf as reached, which a matrix whose +inf means "unreached"
 * cannot say.  Finite weights whose path sum overflows to +inf are accepted, and such a
 * node is reported unreached. */
int safe_nbr_shortpath(safe_ctx *ctx, int64_t n, int64_t n_edges, const int32_t *edge_u,
                       const int32_t *edge_v, const double *edge_w, double cutoff,
                       int keep_distances, safe_nbr **out);

/* node_distance_metric 'diffusion' (additive; the reference's metrics, safepy/safe.py:389-417, count hops or measure a 2-D
 * layout): the truncated random-walk-with-restart kernel of the network and the cosine-normalised distance derived from it.
 * Every operation is f64, rounded, in the order written (no fused multiply-add, no floating-point atomics: identical calls
 * give identical bytes).
 *   Edges: undirected (edge_u[e], edge_v[e]) with weight edge_w[e], or 1 when edge_w is NULL.  Each edge is one CSR entry in
 *     each direction, a self-loop one entry; a row's entries are ordered by (neighbor id, input order); duplicate edges are
 *     all kept and add.
 *   Normalised adjacency: d_i = the row's entry weights added in entry order; r_i = 1.0 / sqrt(d_i), 0 where d_i == 0;
 *     s_ik = (w_ik * r_i) * r_k.
 *   Iteration: X_0 = I; for t = 0 .. steps-1: acc = 0.0, then over row i's entries in order acc = acc + s_ik * X_t[k][j];
 *     X_{t+1}[i][j] = beta * acc for j != i and alpha + beta * acc for j == i, alpha = restart, beta = 1.0 - alpha.
 *     K = X_steps  (in exact arithmetic alpha * sum_{t < steps} (beta S)^t + (beta S)^steps: the walks of at most `steps`
 *     steps, the restart-weighted series with its last term at full weight; it tends to alpha * inv(I - beta S)).
 *   Distance: for i != j, a = min(i, j), b = max(i, j): D[i][j] = +inf (unreached) if K[a][b] == 0, else
 *     1.0 - K[a][b] / sqrt(K[a][a] * K[b][b]) with negative results set to 0.0; D[i][i] = 0.0.  D is exactly symmetric.
 * A[i][j] = (D[i][j] <= cutoff and reached), the diagonal always.  The handle keeps the distances exactly as a
 * safe_nbr_shortpath handle with keep_distances does (D where A is 1, +inf elsewhere; cutoff = +inf keeps every reached
 * pair), so safe_nbr_distances, safe_nbr_distance_select, safe_nbr_row_distance_select, safe_nbr_from_distances_rows and
 * safe_nbr_weights_from_distances serve it unchanged.  kernel_out_host: f64 [n,n] row-major or NULL; receives K.
 * SAFE_E_INVALID: restart outside (0, 1), steps < 1, a NaN cutoff, an edge id outside [0, n), a negative, NaN or infinite
 * weight (zero is allowed).  SAFE_E_UNSUPPORTED: n > SAFE_SELECT_MAX_NODES.  A refused call writes nothing and leaves *out
 * untouched.  Device memory at peak: three n x n f64 matrices (two scratch iterates, released on every return path, and the
 * kept matrix).  Synchronous on the context's stream.  safe_last_diffusion_stats: the time (ms) of all step launches, their
 * number, and the time of the distance transform in the context's last call. */
int safe_nbr_diffusion(safe_ctx *ctx, int64_t n, int64_t n_edges, const int32_t *edge_u, const int32_t *edge_v,
                       const double *edge_w, double restart, int steps, double cutoff, double *kernel_out_host,
                       safe_nbr **out);
int safe_last_diffusion_stats(safe_ctx *ctx, double *steps_ms, int *steps, double *transform_ms);

/* Membership supplied by the caller as the reference's own layout: self.neighborhoods,
 * int64 [n,n] row-major with entries in {0,1} (safe.py:387,430).  Any other value is
 * SAFE_E_VALUE. */
int safe_nbr_from_dense_i64(safe_ctx *ctx, const int64_t *a_host, int64_t n, safe_nbr **out);
/* Optional hint: the 2-D layout the membership was derived from ([n,2] row-major, the x/y node
 * attributes read at safepy/safe.py:393-396).  Only used to renumber nodes along a
 * space-filling curve for the block-sparse matrix-core kernel; results never depend on it.
 * safe_nbr_euclidean records its own xy; without a layout the order is Cuthill-McKee. */
int safe_nbr_set_layout(safe_nbr *nbr, const double *xy_host);
/* Number of stored 256-row x 32-column blocks of the block-sparse membership used by the
 * matrix-core permutation kernel (0 until that kernel has run once on the handle): the
 * algorithmic GEMM size for roofline reporting. */
int safe_nbr_block_count(const safe_nbr *nbr, int64_t *blocks);
/* Of those blocks' 32-row x 32-column pieces (8 per block), the ones that hold at least one member: the kernel issues
 * matrix-core instructions for these only, so the EXECUTED operation count of a call is pieces x 32 x 32 x columns x slices
 * x (permutations + 1) x 2 (roofline reporting; 0 until the kernel has run once on the handle). */
int safe_nbr_piece_count(const safe_nbr *nbr, int64_t *pieces);
int safe_nbr_destroy(safe_nbr *nbr);
int safe_nbr_info(const safe_nbr *nbr, int64_t *n, int64_t *nnz, int64_t *max_row_count);
/* self.neighborhoods in the reference layout: int64 [n,n] row-major (safe.py:430). */
int safe_nbr_to_dense_i64(safe_nbr *nbr, int64_t *out_host);
int safe_nbr_to_dense_i64_dev(safe_nbr *nbr, int64_t *out_dev);
/* np.sum(neighborhoods, axis=1) (safe.py:423). */
int safe_nbr_row_counts(safe_nbr *nbr, int64_t *out_host);
/* CSR view (row_ptr [n+1], col [nnz], ascending columns). */
int safe_nbr_csr(safe_nbr *nbr, int32_t *row_ptr_host, int32_t *col_host);
/* Dense f64 [n,n] distances of a shortest-path handle built with keep_distances
 * (inf where unreached).  SAFE_E_INVALID if distances were not kept. */
int safe_nbr_distances(safe_nbr *nbr, double *out_host);

/* Order statistics of the pairwise node distances, for the radius types the reference reads and then ignores
 * (neighborhood_radius_type 'percentile': safepy/safe.py:377-381, 389-410; safe_default.ini:13).  The multiset is the
 * distances of the unordered node pairs i < j, never stored: exact radix selection over the f64 bit patterns, recomputed
 * (or re-read) in every pass.  out_host[t] = the element of rank ranks[t] (0-based) of the ascending multiset; ranks need
 * not be sorted and may repeat; any number of ranks (they are served SAFE_SELECT_SLOTS distinct prefixes per sweep);
 * n_ranks = 0 only counts.  A rank outside [0, count) is SAFE_E_INVALID (the count is still delivered), n above
 * SAFE_SELECT_MAX_NODES is SAFE_E_UNSUPPORTED (a call sees fewer than 2^32 pairs).  Synchronous on the context's stream.
 *
 * safe_pair_distance_select_xy (safepy/safe.py:377-381, 389-410; safe_default.ini:13): 'euclidean' -- the multiset is
 *   scipy.spatial.distance.pdist(xy), sqrt(dx*dx + dy*dy) with every operation rounded to f64, bit for bit; xy_host is
 *   [n,2] row-major, every coordinate finite (SAFE_E_VALUE otherwise); *n_pairs = n (n - 1) / 2.
 * safe_nbr_distance_select (safepy/safe.py:377-381, 389-410; safe_default.ini:13): the shortest-path metrics -- the
 *   multiset is D[i][j], i < j, D[i][j] finite, of the matrix a safe_nbr_shortpath handle kept (row i = the search from
 *   source i), read in place on the device; *n_finite_pairs = their number.  SAFE_E_INVALID if the handle kept none. */
#define SAFE_SELECT_MAX_NODES 65536
#define SAFE_SELECT_SLOTS 4
int safe_pair_distance_select_xy(safe_ctx *ctx, const double *xy_host, int64_t n, const int64_t *ranks, int64_t n_ranks,
                                 double *out_host, int64_t *n_pairs);
int safe_nbr_distance_select(safe_nbr *nbr, const int64_t *ranks, int64_t n_ranks, double *out_host,
                             int64_t *n_finite_pairs);

/* neighborhood_radius_type 'nearest' (additive; the reference has one radius for the whole network, safepy/safe.py:369-430):
 * every node's neighborhood reaches to its k-th nearest other node.  With D the node-distance matrix of the metric and
 * cand_i = { D[i][j] : j != i } (node i is left out by index, a coincident node counts; for a kept matrix only the finite
 * entries), the radius of row i is r_i = sorted(cand_i)[min(k, |cand_i|) - 1], and 0.0 where cand_i is empty.  Membership is
 * A[i][j] = (D[i][j] <= r_i): the diagonal always, every tie at the k-th distance, never an unreached node; A need not be
 * symmetric.  The selection is K3's radix selection per row, one launch.  All four are synchronous on the context's stream.
 *
 * safe_row_distance_select_xy (safepy/safe.py:369-430): 'euclidean' -- D = squareform(pdist(xy)), bit for bit; xy_host is
 *   [n,2] row-major, every coordinate finite (SAFE_E_VALUE otherwise); k < 1 is SAFE_E_INVALID; radii_out_host is f64 [n].
 * safe_nbr_row_distance_select (safepy/safe.py:369-430): the shortest-path metrics -- D is the matrix a safe_nbr_shortpath
 *   handle kept (row i = the search from source i), read in place.  SAFE_E_INVALID if the handle kept none, or k < 1.
 * safe_nbr_euclidean_rows (safepy/safe.py:369-430): the handle of A[i][j] = (D_ij <= radii[i]) for D = squareform(pdist(xy));
 *   a NaN or negative radius is SAFE_E_VALUE, +inf takes every node.
 * safe_nbr_from_distances_rows (safepy/safe.py:369-430): a new handle of A[i][j] = (D[i][j] <= radii[i], D[i][j] reached)
 *   from the matrix src_nbr kept, on src_nbr's context; src_nbr is left as it was.  keep_distances != 0: the new handle
 *   keeps D[i][j] where A[i][j] = 1 and +inf elsewhere (what a cutoff handle keeps).  SAFE_E_INVALID if src_nbr kept no
 *   distances, SAFE_E_VALUE on a NaN or negative radius.
 * A refused call writes nothing. */
int safe_row_distance_select_xy(safe_ctx *ctx, const double *xy_host, int64_t n, int64_t k, double *radii_out_host);
int safe_nbr_row_distance_select(safe_nbr *nbr, int64_t k, double *radii_out_host);
int safe_nbr_euclidean_rows(safe_ctx *ctx, const double *xy_host, int64_t n, const double *radii_host, safe_nbr **out);
int safe_nbr_from_distances_rows(safe_nbr *src_nbr, const double *radii_host, int keep_distances, safe_nbr **out);

/* The fused all-pairs kernel on its own (compute_node_distances for 'euclidean', and
 * the K1 roofline bench): xy_dev [n,2]; mask_out_dev int64 [n,n] and/or dist_out_dev
 * f64 [n,n]; either may be NULL.  Same arithmetic as safe_nbr_euclidean
 * (safepy/safe.py:397-399). */
int safe_euclidean_dense_dev(safe_ctx *ctx, const double *xy_dev, int64_t n, double nr,
                             int64_t *mask_out_dev, double *dist_out_dev);
/* Replaces calculate_edge_lengths (safepy/safe_io.py:311-333): length[e] =
 * sqrt(dx*dx + dy*dy) of the edge's end points, without the N x N detour. */
int safe_edge_lengths(safe_ctx *ctx, const double *xy_host, int64_t n, int64_t n_edges,
                      const int32_t *edge_u, const int32_t *edge_v, double *out_host);

/* Spring-embedded layout: the nx.spring_layout(G, k=0.2, iterations=100, seed=...) of apply_network_layout
 * (safepy/safe_io.py:288-308), before networkx's rescale_layout.  Restates networkx 3.4.2's
 * _fruchterman_reingold (dtype SAFE_DTYPE_F64, what it runs below 500 nodes) or _sparse_fruchterman_reingold
 * (SAFE_DTYPE_F32, 500 nodes and more) operation by operation, with each node's force summed over the other
 * nodes in node order, so the coordinates equal networkx's bit for bit.  The adjacency is the CSR row_ptr [n+1],
 * col [nnz] (strictly increasing columns per row, both directions of every edge; SAFE_E_VALUE otherwise) with
 * weights weight [nnz] (NULL = 1; rounded to f32 in the F32 form); pos0_f64 [n,2] row-major is the initial
 * seed.rand(n, 2) draw.  pos_out [n,2] receives the positions in the form's precision (f32 values widened
 * exactly), *iterations_run how many iterations ran before norm(delta_pos) / n < threshold stopped them (that
 * norm is summed in another order than numpy's, so the stop can differ only when the ratio lies within rounding
 * of the threshold).  n <= 65536 (SAFE_E_UNSUPPORTED beyond).  Host pointers; synchronous. */
int safe_layout_spring(safe_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col, const double *weight,
                       int dtype, const double *pos0_f64, double k, int iterations, double threshold,
                       double *pos_out, int *iterations_run);

/* Kamada-Kawai layout: the nx.kamada_kawai_layout(G) of apply_network_layout (safepy/safe_io.py:288-308; networkx 3.4.2
 * kamada_kawai_layout -> _kamada_kawai_solve -> _kamada_kawai_costfn, dim = 2).  A handle holds what _kamada_kawai_solve
 * prepares once -- invdist = 1 / (dist_mtx + eye * 1e-3) and its transpose, 16 n^2 bytes of device memory -- and
 * safe_kk_eval is _kamada_kawai_costfn: cost and gradient at a position vector, every operation rounded as NumPy rounds
 * it and every sum taken in NumPy's order (each node's two einsum sums over the other nodes in node order; np.sum(offset**2)
 * in 8192-element buffers, each summed pairwise), so both equal networkx's bit for bit, NaN entries for coincident nodes
 * included (their payloads are not specified).  The minimiser stays the caller's (scipy.optimize.minimize, L-BFGS-B).
 *
 * safe_kk_create_host (safe_io.py:288-308; kamada_kawai_layout's dist_mtx): dist_host f64 [n, n] row-major,
 *   dist[i][j] = preferred distance from node i to node j, read as given ([i][j] and [j][i] are two values); +inf counts
 *   as networkx's 1e6 for an unreached node.
 * safe_kk_create_nbr (safe_io.py:288-308; kamada_kawai_layout's dict(nx.shortest_path_length(G, weight=weight))): the
 *   distances a safe_nbr_shortpath handle of the same context kept (keep_distances != 0; cutoff = +inf for all pairs),
 *   read on the device -- no n^2 transfer.  SAFE_E_INVALID if the handle kept none.  The membership handle may be destroyed
 *   afterwards.
 * Both: a NaN or negative distance is SAFE_E_VALUE, n > SAFE_KK_MAX_NODES is SAFE_E_UNSUPPORTED (64 GiB of matrices at the
 *   limit), n >= 1.  Enqueued on the context's stream; synchronise.
 * safe_kk_eval (safe_io.py:288-308; _kamada_kawai_costfn): pos_host f64 [n, 2] row-major in, *cost and grad_host f64 [n, 2]
 *   out.  Synchronous on the context's stream.  No atomics: repeated calls give identical bits. */
#define SAFE_KK_MAX_NODES 65536
int safe_kk_create_host(safe_ctx *ctx, const double *dist_host, int64_t n, safe_kk **out);
int safe_kk_create_nbr(safe_ctx *ctx, safe_nbr *nbr, safe_kk **out);
int safe_kk_eval(safe_kk *kk, const double *pos_host, double *cost, double *grad_host);
int safe_kk_destroy(safe_kk *kk);

/* --------------------------------------------------------------- attributes ---- */
/* self.node2attribute (safepy/safe_io.py:410): [n,m], f32 or f64, NaN = missing, with
 * element strides (row_stride, col_stride): (m,1) for C order, (1,n) for Fortran order.
 * The _host form uploads a copy; the _dev form borrows the caller's device buffer, which
 * must outlive the handle.  Additive (the reference's loader hands over f32, safe_io.py:361, and the
 * upload of a 0/1 matrix is most of a hypergeometric call, safe.py:556-608): the _host form also
 * takes SAFE_DTYPE_U8 -- one byte per value over the link, widened to f32 on the device. */
int safe_attr_create_host(safe_ctx *ctx, const void *b_host, int dtype, int64_t n, int64_t m,
                          int64_t row_stride, int64_t col_stride, safe_attr **out);
int safe_attr_create_dev(safe_ctx *ctx, const void *b_dev, int dtype, int64_t n, int64_t m,
                         int64_t row_stride, int64_t col_stride, safe_attr **out);
/* Additive: self.node2attribute given SPARSE -- the compressed-sparse-column form annotation matrices are built and stored
 * in (the reference's own GO builder produces a sparse frame before read_attributes densifies it, safepy/safe_io.py:410) --
 * and expanded on the device: the upload is 8 (m + 1) + 4 nnz bytes (+ the values) instead of n m values.  The handle owns
 * a dense Fortran-order matrix D of `dtype` (SAFE_DTYPE_F32 when values is NULL: every stored entry is 1) and no later
 * call can tell it from safe_attr_create_host of D:
 *   D is 0 everywhere, with values[k] at (indices[k], j) for indptr[j] <= k < indptr[j + 1]; stored zeros and stored NaNs
 *   are legal and mean 0 and NaN; every row i with missing_rows[i] != 0 (NULL: none) is NaN in every column -- the nodes
 *   read_attributes fills with fill_value = NaN (safe_io.py:386-390).
 * Contract on the input: indptr[0] == 0, indptr[m] == nnz, indptr non-decreasing; row indices strictly increasing inside a
 * column and in [0, n); nnz < 2^31.  A kernel checks it on the device before anything is scattered; a violation returns
 * SAFE_E_VALUE with a message naming the first rule broken (in the order above) and creates no handle.
 * When no stored value differs from 1 and no stored entry lies on a missing row, the input already is the list of ones
 * per column that the scatter form of the permutation test reads, and is kept as such (no scan of D on first use).
 * Enqueued on the context's stream; synchronises (the verdict is read back, and the staging memory goes back to the
 * context's pool before the call returns). */
int safe_attr_create_csc_host(safe_ctx *ctx, int64_t n, int64_t m, int64_t nnz, const int64_t *indptr /*[m+1]*/,
                              const int32_t *indices /*[nnz]*/, const void *values /*[nnz] or NULL*/, int dtype /*F32|F64*/,
                              const uint8_t *missing_rows /*[n] or NULL*/, safe_attr **out);
int safe_attr_destroy(safe_attr *attr);
/* read_attributes on the device (safepy/safe_io.py:386-390 `node2attribute.reindex(index=
 * node_label_order, fill_value=fill_value)` + `.values` at :410): uploads the file's
 * [n_labels, m] table (f32 or f64, C or Fortran order by element strides) once, gathers its
 * rows into network node order -- row_map_host[i] = table row of node i, -1 = label not in
 * the file (filled with fill_value), -2 = masked duplicate node (NaN, safe_io.py:394-404) --
 * and returns the aligned matrix as a device-resident handle, laid out C (out_order 0) or
 * Fortran (1).  If out_host is not NULL the aligned matrix (same dtype and order) is also
 * copied there: that is self.node2attribute. */
int safe_attr_reindex(safe_ctx *ctx, const void *table_host, int dtype, int64_t n_labels, int64_t m,
                      int64_t row_stride, int64_t col_stride, const int64_t *row_map_host, int64_t n,
                      double fill_value, int out_order, void *out_host, safe_attr **out);
/* The value census read_attributes logs (safepy/safe_io.py:426-429): #NaN, #zeros,
 * #positives, #negatives of the whole matrix in one pass. */
int safe_attr_value_counts(safe_attr *attr, int64_t *n_nan, int64_t *n_zero, int64_t *n_positive,
                           int64_t *n_negative);
/* background='network' (safepy/safe.py:449-451): NaN -> 0 in place on the device copy. */
int safe_attr_nan_to_zero(safe_attr *attr);
/* Copies the device matrix (its own dtype and order) to the host. */
int safe_attr_download(safe_attr *attr, void *out_host);
/* Whole-matrix facts compute_pvalues needs before dispatch (safepy/safe.py:453-463):
 *   n_other   = #(non-NaN values not in {0,1})          -> 'auto' rule (safe.py:461)
 *   max_nan_col = max over columns of the NaN count      -> >50% warning (safe.py:454-459)
 *   n_rows_with_value = #rows with >= 1 non-NaN value    -> hypergeometric N (safe.py:574-578)
 *   n_non_integer = #(non-NaN values that are not integers) */
int safe_attr_stats(safe_attr *attr, int64_t *n_other, int64_t *max_nan_col,
                    int64_t *n_rows_with_value, int64_t *n_non_integer);
/* row_has_value[i] = 1 iff row i has >= 1 non-NaN value: indx_vals of
 * safepy/safe_extras.py:51 and nodes_not_nan of safepy/safe.py:574. */
int safe_attr_row_flags(safe_attr *attr, uint8_t *out_host);
/* nansum of every column in f64 (np.nansum(node2attribute, axis=0), safepy/safe.py:583: the hypergeometric N_in_group): the sums the
 * statistics pass left on the device, out_host f64 [m].  Integer-valued columns are exact; other values add in an order
 * that depends on the layout.  Host output: synchronises. */
int safe_attr_column_sums(safe_attr *attr, double *out_host);
/* Exact first and second moments of columns [col0, col1) over the rows the randomization route permutes (row_has_value = 1:
 * indx_vals of safepy/safe_extras.py:51; a NaN cell inside them counts as 0, safe_extras.py:10), host f64 [col1 - col0] each:
 *   mean = column_sum / n_rows_with_value (0 when no row has a value)
 *   css  = sum over those rows of (b - mean)^2, centred, in a second pass; exactly 0 when the column's min equals its max
 * Values are widened to f64 before any arithmetic; the summation order is fixed (no floating-point atomics), so two calls
 * give the same bits.  Runs on the context's stream; host outputs: synchronises. */
int safe_attr_column_moments(safe_attr *attr, int64_t col0, int64_t col1, double *mean_host, double *css_host);
/* Override the row flags (attribute-sharded multi-GPU runs must use the flags of the
 * FULL matrix, not of the local column shard). */
int safe_attr_set_row_flags(safe_attr *attr, const uint8_t *flags_host);
/* Additive (attribute_transform = 'rank'): every column of `src` replaced by its midranks.  *out is a new handle that owns a
 * dense f64 matrix R of the same [n, m] in Fortran order, and no later call can tell it from safe_attr_create_host of R
 * (statistics, column sums, moments and support lists are built lazily, as for any handle).  For every column j:
 *   R[i, j] = NaN where src is NaN, else the midrank of the value among the column's non-NaN values: the mean of the 1-based
 *   positions its tie group takes in ascending order -- scipy.stats.rankdata(col, method='average', nan_policy='omit'), bit for
 *   bit (a multiple of 0.5).
 * Equality is IEEE equality of the values widened to f64: -0.0 ties with +0.0, -inf / +inf rank at the ends, subnormals and values
 * one ulp apart are distinct.
 * src: any handle -- f32, f64, u8 widened to f32 on upload, either element order, made by _host, _dev, _csc_host or _reindex --
 * and is not modified.  The new handle inherits src's row flags as they are, flags installed by safe_attr_set_row_flags
 * included (the set of NaN cells is unchanged; a column shard of a multi-GPU run keeps the full matrix's flags); where src has
 * none yet, the new handle finds its own on first use, and they are the same.
 * Any n and m a handle holds; the rows of a column are sorted in chunks of SAFE_RANK_CHUNK and no limit on n comes from the
 * chunk (n < 2^30).  Runs on the context's stream and synchronises.  Scratch (8 m ceil(n / SAFE_RANK_CHUNK) SAFE_RANK_CHUNK
 * bytes) belongs to the call and is gone on every return path; R's block is the only allocation that survives.  A NULL argument
 * is SAFE_E_INVALID and creates nothing (*out = NULL on every failure).  safe_last_kernel_stats names
 * k_rank_keys+k_rank_sort+k_rank_emit; safe_last_rank_stats gives the three kernels' times (ms) of the context's last call. */
#define SAFE_RANK_CHUNK 4096
int safe_attr_rank(safe_attr *src, safe_attr **out);
int safe_last_rank_stats(safe_ctx *ctx, double *keys_ms, double *sort_ms, double *emit_ms);

/* ------------------------------------------------------------ permutations ---- */
/* The row-permutation stream of run_permutations (safepy/safe_extras.py:46-58):
 * np.random.seed(seed) (legacy MT19937 init_genrand) followed by num_permutations calls
 * of np.random.permutation(indx_vals) (masked-rejection Fisher-Yates), applied
 * cumulatively; movable_host[i] != 0 marks indx_vals.  has_seed == 0 seeds from OS
 * entropy (random_seed=None).  The result is the composed table cur[p][i] with
 * permuted_matrix_p = B[cur[p]], resident on the device.  Split of the work: one host thread runs
 * MT19937 and the rejection chain (how many words a shuffle consumes depends on its rejections:
 * the one sequential part) and ships the accepted swap targets; the swaps are replayed and the
 * tables composed on the device, chunk by chunk, while the enrichment kernels of earlier chunks run. */
int safe_perms_create(safe_ctx *ctx, int64_t n, const uint8_t *movable_host,
                      int64_t num_permutations, int has_seed, uint32_t seed, safe_perms **out);
int safe_perms_destroy(safe_perms *perms);
/* Copy table rows [p0,p1) to host as int32 [p1-p0, n] (tests). */
int safe_perms_read(safe_perms *perms, int64_t p0, int64_t p1, int32_t *out_host);
/* The same handle from a table the CALLER supplies instead of the legacy stream -- the `perm` of
 * safepy/safe_extras.py:58 produced elsewhere (an external RNG, a recorded run): perm_idx_host is int32
 * [num_permutations, n] row-major, COMPOSED like the tables above: row p is the index vector with
 * permuted_matrix_p = B[perm_idx[p]] (for the reference's cumulative in-place shuffle that is
 * cur_p = cur_{p-1}[...] of SURVEY A.3, not the single draw).  Every row must be a permutation of
 * 0..n-1 (SAFE_E_VALUE otherwise). */
int safe_perms_create_from_table(safe_ctx *ctx, int64_t n, int64_t num_permutations,
                                 const int32_t *perm_idx_host, safe_perms **out);
/* Permutations [p0, p1) of an existing handle as a handle of their own (device-to-device copy).  The permutation-axis
 * split of safepy/safe.py:489-519 (the reference hands each worker process num_permutations / processes permutations;
 * its workers reseed identically, so they repeat one another -- here every rank draws the ONE cumulative stream of
 * safe_extras.py:46-58 and tests its own range of it, and the ranks' counts add up to the single-process counts). */
int safe_perms_slice(safe_perms *perms, int64_t p0, int64_t p1, safe_perms **out);
/* UNSEEDED runs (random_seed=None -- the reference's default, safepy/safe.py:88; np.random.seed(None) at safe_extras.py:46 takes
 * OS entropy, so there is no stream to reproduce): the tables are generated ON THE DEVICE.  The reference's cumulative in-place
 * shuffles (safe_extras.py:58) make the composed tables i.i.d. uniform permutations of the movable rows, so each table row is
 * drawn directly: one lane per permutation runs Fisher-Yates in LDS with Philox4x32-10 words (key = `key`, counter =
 * permutation, word block) and unbiased bounded draws (Lemire's multiply-shift with rejection).  No host thread, nothing
 * sequential across permutations; every rank of a sharded run generates identical tables from the same key.  num movable rows
 * <= 65535.  The same arguments and the same handle as safe_perms_create otherwise; tables depend on (key, movable rows,
 * num_permutations index) only -- restated in oracle/safe_oracle.py for the tests. */
int safe_perms_create_device(safe_ctx *ctx, int64_t n, const uint8_t *movable_host, int64_t num_permutations,
                             uint64_t key, safe_perms **out);
/* RESTRICTED permutations: the device stream of safe_perms_create_device with the rows shuffled only inside strata of
 * comparable nodes (the strata= / blocks= argument of permutation-test packages).  stratum_host is int32 [n]: the label of
 * every row, >= 0, read only where the row is movable.  The movable rows are listed stratum by stratum -- strata in ascending
 * label order, rows ascending inside a stratum -- and row q of the table shuffles every stratum on its own with the device
 * stream's algorithm applied to that stratum's element list: each element draws one of 64 buckets, buckets keep ascending
 * element order, Fisher-Yates runs from the top inside each bucket, Lemire draws with the same fallback counters; the element
 * index e and the step i are local to the stratum, and the stratum's rank s (0-based position among the distinct labels of
 * the movable rows) goes into word 2 of every Philox counter: (s << 16) | tag for the tags 0xB0C7, 0x5AFE, 0xFA11.  So a
 * partition with ONE stratum gives the tables of safe_perms_create_device with the same key bit for bit, and the tables
 * depend on (key, movable rows, partition, permutation index) only.  Rows that are not movable and the padding entry n map to
 * themselves; a stratum of one row stays put.  Rows of the table are i.i.d. (no composition step).  The handle is the one
 * safe_perms_create_device returns (32-bit and, for n < 65535, 16-bit table, every stage complete behind the launch, role 3
 * in safe_perms_timing); it never enters or consults the resident-table reuse of seeded handles.
 * Refusals (nothing written, *out = NULL): more than 65535 movable rows SAFE_E_UNSUPPORTED; a negative label on a movable
 * row SAFE_E_VALUE; NULL arguments, n out of range, a negative count SAFE_E_INVALID.  num_permutations = 0 and no movable row
 * at all are valid, as for safe_perms_create_device. */
int safe_perms_create_device_strata(safe_ctx *ctx, int64_t n, const uint8_t *movable_host, const int32_t *stratum_host,
                                    int64_t num_permutations, uint64_t key, safe_perms **out);
/* One permutation stream per NODE (multi-GPU runs; the reference's workers each repeat the whole stream,
 * safepy/safe.py:489-519, 1339-1353).  The stream of safe_extras.py:46-58 is sequential, so a rank cannot draw "its part":
 * safe_ctx_share_stream attaches the context to a shared-memory ring named `name` (the same string on every rank of the
 * node, unique per job; capacity_bytes of chunk slots), local rank 0 being the node's producer.  safe_perms_create_shared
 * then behaves exactly like safe_perms_create -- same arguments, same tables -- but only the producer runs the draw
 * thread; it publishes each pipeline chunk's accepted swap targets (2 bytes each) and the other ranks block (futex, no CPU)
 * until a chunk is there, copy it and upload it; every rank replays the swaps and composes the tables on its own device.  The call is COLLECTIVE over the ranks of the node: same n, movable rows and permutation count,
 * same order of calls (checked: SAFE_E_VALUE otherwise; waits time out after SAFE_HIP_RING_TIMEOUT_S, default 120 s).  The
 * seed is the producer's.  When a chunk (128 x n x 2 bytes; 4 beyond 65535 rows) does not fit the ring twice, or the context shares no
 * stream, every rank silently draws for itself (decided from n and the capacity alone, hence identically everywhere). */
int safe_ctx_share_stream(safe_ctx *ctx, const char *name, int local_rank, int local_world, int64_t capacity_bytes);
int safe_ctx_unshare_stream(safe_ctx *ctx);
int safe_perms_create_shared(safe_ctx *ctx, int64_t n, const uint8_t *movable_host, int64_t num_permutations,
                             int has_seed, uint32_t seed, safe_perms **out);
/* Host-side timing of a handle's stream, ms: out5[0] = time the draw thread spent drawing, [1] = handle creation -> last
 * draw finished, [2] = creation -> last chunk's table kernels enqueued, [3] = time this rank blocked waiting for the
 * node's producer, [4] = role (0 own stream, 1 producer of a shared stream, 2 consumer, 3 generated on the device).  For
 * bench reporting. */
int safe_perms_timing(safe_perms *perms, double *out5);
/* The twin chain of a seeded handle (np.random.seed / np.random.permutation, safepy/safe_extras.py:46,58, drawn by two host
 * threads at once on a shared host: whichever finishes a pipeline chunk first publishes it): *twin_active = it runs for this
 * handle (opt-in: SAFE_HIP_DRAW_TWIN=1, single-process seeded calls with polling waits -- measured no better than one thread), *chunks = chunks published
 * so far, *chunks_won_by_twin = how many of them came from the second thread.  For bench reporting. */
int safe_perms_twin_stats(safe_perms *perms, int *twin_active, int64_t *chunks, int64_t *chunks_won_by_twin);
/* The ring by itself (host memory only, no device): what safe_perms_create_shared runs on, exported so that the
 * multi-process protocol can be tested on a host without GPUs.  local rank 0 creates, the others attach;
 * safe_ring_begin opens the next call on either side (producer: waits until every consumer has left the previous one;
 * consumer: waits for the producer's announcement and checks n / k / count / movable_hash against it);
 * safe_ring_publish / safe_ring_fetch move chunk `chunk` (in order); safe_ring_end leaves the call. */
int safe_ring_open(const char *name, int local_rank, int local_world, int64_t capacity_bytes, safe_ring **out);
int safe_ring_close(safe_ring *ring);
int safe_ring_begin(safe_ring *ring, int64_t n, int64_t k, int64_t count, uint64_t movable_hash, int64_t slot_bytes);
int safe_ring_publish(safe_ring *ring, int64_t chunk, const void *src_host, size_t bytes);
int safe_ring_fetch(safe_ring *ring, int64_t chunk, void *dst_host, size_t bytes);
int safe_ring_end(safe_ring *ring);
/* Host-only: the raw stream, for pinning against numpy (no device needed).  Writes
 * count permutations of values[0..n_items) back to back into out[count*n_items]. */
int safe_rng_permutations_host(uint32_t seed, const int64_t *values, int64_t n_items,
                               int64_t count, int64_t *out);

/* -------------------------------------------------------------- enrichment ---- */
/* Replaces compute_neighborhood_score (safepy/safe_extras.py:6-33).  Columns
 * [col0,col1) of the attribute handle; out_dev is f64 [n, col1-col0] row-major. */
int safe_score(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int score_type,
               int64_t col0, int64_t col1, double *out_dev);

/* Replaces run_permutations (safepy/safe_extras.py:36-70): counts_neg/counts_pos as
 * f64 [n, col1-col0] (number of permutations with permuted score <= / >= observed);
 * ns_dev (observed score) may be NULL. */
int safe_permtest_counts(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, safe_perms *perms,
                         int score_type, int64_t col0, int64_t col1, double *ns_dev,
                         double *counts_neg_dev, double *counts_pos_dev);

/* Replaces compute_pvalues_by_randomization + the binarisation of compute_pvalues
 * (safepy/safe.py:496-554, 468-472; FDR branch excluded): all outputs f64
 * [n, col1-col0] row-major on the device, num_enriched_dev f64 [col1-col0].
 * nes_table_host: optional [P+1] table with nes_table[k] = -log10(k/P), k >= 1, and
 * nes_table[0] = -log10(1/P) evaluated by the caller's libm (NumPy) so NES matches the
 * caller's log10 bit for bit; NULL = use the library's log10. */
int safe_randomization(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, safe_perms *perms,
                       int score_type, int sign_mode, double enrichment_threshold,
                       const double *nes_table_host, int64_t col0, int64_t col1,
                       double *ns_dev, double *pvalues_neg_dev, double *pvalues_pos_dev,
                       double *nes_dev, double *nes_binary_dev, double *num_enriched_dev);

/* Replaces compute_pvalues_by_hypergeom + the binarisation (safepy/safe.py:573-608,
 * 468-472; FDR branch excluded).  n_rows_with_value is the population size of
 * safe.py:578 (from safe_attr_stats of the FULL matrix). */
int safe_hypergeom(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, double enrichment_threshold,
                   int64_t col0, int64_t col1, double *pvalues_pos_dev, double *nes_dev,
                   double *nes_binary_dev, double *num_enriched_dev);

/* multiple_testing=True (safepy/safe.py:536-542 and 599-605): Benjamini-Hochberg adjustment of
 * every row of the p-value matrices across its m attributes -- statsmodels'
 * fdrcorrection(row)[1], operation by operation -- IN PLACE on pvalues_neg_dev / pvalues_pos_dev
 * (f64 [n,m] row-major), then NES, nes_binary and the per-attribute counts recomputed from the
 * adjusted values (safe.py:546-554 / 608, 468-472).  num_permutations > 0: randomization form
 * (zero p-values become 1/num_permutations inside the logarithm, sign_mode combines the two
 * sides); num_permutations == 0: hypergeometric form (nes = -log10 pvalues_pos; pvalues_neg_dev
 * may be NULL).  A row needs all of its attributes: under attribute sharding this runs after the
 * p-value blocks have been gathered.  With num_permutations > 0 the p-values are normally
 * count / num_permutations (what safe_randomization and safe_outputs_from_* write): both matrices are
 * checked read-only, and if every entry is such a ratio the rows are adjusted from their histogram
 * over the counts, without a sort; otherwise (a caller's own values) they are sorted like the
 * hypergeometric form.  Nothing is modified before the form is chosen.  In every form a NaN of either
 * sign and any payload turns its whole row into 0x7FF8... (np.argsort puts every NaN last, np.minimum
 * carries it through the row) and -0.0 is the value 0.0, as NumPy sorts it (its adjusted value is +0.0);
 * negative p-values other than -0.0 are the caller's error and not defined. */
int safe_fdr_adjust(safe_ctx *ctx, int64_t n, int64_t m, int64_t num_permutations, int sign_mode,
                    double enrichment_threshold, double *pvalues_neg_dev, double *pvalues_pos_dev, double *nes_dev,
                    double *nes_binary_dev, double *num_enriched_dev);

/* Benjamini-Hochberg adjustment of every row of ONE matrix (f64 [n,m] row-major), in place: what safe_fdr_adjust with
 * num_permutations = 0 does to pvalues_pos_dev, without the NES epilogue (the rows are sorted; no histogram form). */
int safe_fdr_adjust_rows(safe_ctx *ctx, int64_t n, int64_t m, double *p_dev);

/* safe_fdr_adjust with the family named by `scope` (additive; the reference adjusts rows only, safepy/safe.py:536-542, 599-605):
 *   SAFE_FDR_SCOPE_ROWS  np.apply_along_axis(lambda r: fdrcorrection(r)[1], 1, p): safe_fdr_adjust itself, the same bytes
 *   SAFE_FDR_SCOPE_COLS  the same along axis 0: one attribute's column across the n neighborhoods
 *   SAFE_FDR_SCOPE_ALL   fdrcorrection(p.ravel())[1].reshape(p.shape): the n m tests as one family
 * in place on pvalues_neg_dev / pvalues_pos_dev, then NES, nes_binary and the per-attribute counts by the epilogue of
 * safe_fdr_adjust (safe.py:546-554 / 608, 468-472).  The NaN rule of safe_fdr_adjust holds for the family: a NaN of either sign
 * and any payload turns its whole column -- with SAFE_FDR_SCOPE_ALL the whole matrix -- into 0x7FF8...; -0.0 is the value 0.0.
 * With num_permutations > 0 both matrices are checked read-only first; if every entry is a count ratio the families are
 * adjusted from histograms over the counts (columns: num_permutations <= 4095; whole matrix: <= 16383), otherwise they are
 * sorted, and the result is the same.  The whole-matrix sort takes n m < 2^31 entries: beyond that SAFE_E_UNSUPPORTED, before
 * anything is written.  Bad arguments (NULL, n or m < 1, scope outside 0 ... 2, enrichment_threshold outside (0, 1)) are
 * SAFE_E_VALUE, before anything is written. */
int safe_fdr_adjust_scope(safe_ctx *ctx, int64_t n, int64_t m, int64_t num_permutations, int sign_mode,
                          double enrichment_threshold, int scope, double *pvalues_neg_dev, double *pvalues_pos_dev,
                          double *nes_dev, double *nes_binary_dev, double *num_enriched_dev);

/* Benjamini-Hochberg adjustment of ONE matrix (f64 [n,m] row-major) in place along `scope`, without the NES epilogue: the scoped
 * counterpart of safe_fdr_adjust_rows (the two-sided tests call it on both matrices, then safe_hypergeom_outputs).
 * count_denominator = 0: the families are sorted.  count_denominator = P > 0: the caller says the entries are counts / P; the
 * matrix is checked read-only, and anything that is not such a ratio, or a P beyond the count form's limit, goes through the
 * sort with the same result.  Errors as safe_fdr_adjust_scope. */
int safe_fdr_adjust_matrix(safe_ctx *ctx, int64_t n, int64_t m, int scope, int64_t count_denominator, double *p_dev);

/* safe_fdr_adjust_scope / safe_fdr_adjust_matrix with the procedure named by `method` (additive: multiple_testing_method), each
 * statsmodels' multipletests operation by operation on a family of `count` entries (m, n or n m), ps the family sorted as
 * np.argsort does, k = 1 ... count the sorted position:
 *   SAFE_MT_FDR_BH      ps_k / (k / count), running minimum from the right, clamp at 1: the bytes of the safe_fdr_* calls
 *   SAFE_MT_FDR_BY      ps_k / ((k / count) / by_constant), the same scan; by_constant = sum_{i <= count} 1 / i comes from the
 *                       caller as a double (the library sums nothing): not finite or below 1 is SAFE_E_VALUE
 *   SAFE_MT_HOCHBERG    (count - k + 1) ps_k, the same scan
 *   SAFE_MT_HOLM        (count - k + 1) ps_k, running MAXIMUM from the LEFT, clamp
 *   SAFE_MT_BONFERRONI  ps count, clamp: element-wise, no sort, no histogram, no limit on n m
 * by_constant is ignored unless method is SAFE_MT_FDR_BY.  -0.0 is the value 0.0 everywhere.  BH, BY and Hochberg: one NaN turns
 * its whole family into 0x7FF8... (the rule of safe_fdr_adjust).  Holm and Bonferroni: a NaN entry becomes 0x7FF8... on its own
 * and the numbers are adjusted as members of a family of `count` entries, NaNs counted (np.maximum.accumulate from the left never
 * passes a NaN that np.argsort put last).  Forms, stream behaviour, SAFE_HIP_FDR_SORT and refusals are those of the safe_fdr_*
 * counterparts; a method outside 0 ... 4 is SAFE_E_VALUE as well; nothing is written on any refusal. */
#define SAFE_MT_FDR_BH 0
#define SAFE_MT_FDR_BY 1
#define SAFE_MT_HOLM 2
#define SAFE_MT_HOCHBERG 3
#define SAFE_MT_BONFERRONI 4
int safe_mt_adjust_scope(safe_ctx *ctx, int64_t n, int64_t m, int64_t num_permutations, int sign_mode,
                         double enrichment_threshold, int scope, int method, double by_constant, double *pvalues_neg_dev,
                         double *pvalues_pos_dev, double *nes_dev, double *nes_binary_dev, double *num_enriched_dev);
int safe_mt_adjust_matrix(safe_ctx *ctx, int64_t n, int64_t m, int scope, int method, double by_constant,
                          int64_t count_denominator, double *p_dev);

/* The hypergeometric test with BOTH tails, for 0/1 attributes (NaN allowed): what compute_pvalues_by_hypergeom would set if it
 * followed attribute_sign the way the randomization route does (safepy/safe.py:546-554; the reference computes the upper tail
 * only, safe.py:596).  All outputs f64 [n, col1 - col0] row-major, num_enriched_dev f64 [col1 - col0]:
 *   ns          x = A . nan_to_num(B)  (safe.py:593-594; safe_score 'sum')
 *   pvalues_pos P[H >= x] = hypergeom.sf(x - 1, N, K, n), N / K / n as at safe.py:574-590
 *   pvalues_neg P[H <= x] = hypergeom.cdf(x, N, K, n): 0 below the support, 1 at or above its top
 *   nes         -log10 pvalues_pos (SAFE_SIGN_HIGHEST), -log10 pvalues_neg (SAFE_SIGN_LOWEST), the first minus the second
 *               (SAFE_SIGN_BOTH); no 1 / P substitution: p = 0 gives +-inf (safe.py:608)
 *   nes_binary  |nes| > -log10(enrichment_threshold) (safe.py:468-472): decided on p itself for one side, on the difference of the
 *               logarithms in doubles for SAFE_SIGN_BOTH; NaN -> 0.  num_enriched = its column sums.
 * evaluator: 0 = the library chooses, 1 = the table evaluator (one thread per distinct (n, K) pair, both tails in double-double,
 * correctly rounded but for ties; SAFE_E_UNSUPPORTED when the table would exceed 512 MB or the call has fewer than 4 cells per
 * pair), 2 = the per-element evaluator (relative error <= 1e-6 for p >= 1e-290).  A matrix that holds anything but 0, 1 and NaN is
 * SAFE_E_VALUE, reported before anything is launched.  safe_last_kernel_stats names the evaluator: k_hyp_tails_emit<table> or
 * k_hyp_tails_emit<element>. */
int safe_hypergeom_tails(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int sign_mode, double enrichment_threshold,
                         int evaluator, int64_t col0, int64_t col1, double *ns_dev, double *pvalues_neg_dev,
                         double *pvalues_pos_dev, double *nes_dev, double *nes_binary_dev, double *num_enriched_dev);

/* NES, nes_binary and the per-attribute counts from two p matrices (f64 [n,m] row-major, read only) under the rules of
 * safe_hypergeom_tails: what follows safe_fdr_adjust_rows on both matrices when multiple_testing is on. */
int safe_hypergeom_outputs(safe_ctx *ctx, int64_t n, int64_t m, int sign_mode, double enrichment_threshold,
                           const double *pvalues_neg_dev, const double *pvalues_pos_dev, double *nes_dev,
                           double *nes_binary_dev, double *num_enriched_dev);

/* The analytic form of the randomization test for neighborhood_score_type == 'sum' (any attribute values): the null that
 * run_permutations samples (safepy/safe_extras.py:36-70: the rows with a value are shuffled) has closed-form moments, so no
 * permutation is drawn, the result has no seed, and p-values run down to the smallest double instead of 1 / num_permutations.
 * With n_v = n_rows_with_value, mu_j and Q_j the mean and css of safe_attr_column_moments, k_i the members of neighborhood i
 * that have a value, all outputs f64 [n, col1 - col0] row-major, num_enriched_dev f64 [col1 - col0]:
 *   ns          x = A . nan_to_num(B)  (safe_score 'sum')
 *   var         k_i (n_v - k_i) / (n_v (n_v - 1)) * Q_j, rounded in that order
 *   z           (x - k_i * mu_j) / sqrt(var); written to z_dev when it is not NULL
 *   pvalues_pos P[Z >= z], pvalues_neg P[Z <= z] for a standard normal Z: the smaller one is erfc(|z| * sqrt(1/2)) / 2 -- one
 *               erfc per cell -- and the larger one 1 minus that
 *   degenerate  n_v < 2, k_i = 0, k_i = n_v or a constant column (var not positive): every permuted score equals the observed
 *               one, so pvalues_pos = pvalues_neg = 1 and z = 0, the permutation test's own limit
 *   nes, nes_binary, num_enriched: the rules of safe_hypergeom_tails (no 1 / P substitution, p = 0 gives +-inf)
 * safe_last_kernel_stats names k_moments_emit. */
int safe_moments_test(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int sign_mode, double enrichment_threshold,
                      int64_t col0, int64_t col1, double *ns_dev, double *pvalues_neg_dev, double *pvalues_pos_dev,
                      double *nes_dev, double *nes_binary_dev, double *num_enriched_dev, double *z_dev /* may be NULL */);

/* ---- distance-weighted neighborhoods (weights.hip) ---------------------------------------------------------------------
 * A membership handle may carry one weight w_ik >= 0 per member k of row i.  Weights change nothing any entry point above
 * computes on the handle; only the three *_weighted entry points below read them.  All arithmetic is f64, every operation
 * rounded, in the order written (the library is built with -ffp-contract=off).
 *   members     of row i = its CSR entries (safe_nbr_csr), in ascending column order
 *   D[i,k]      the node distance: sqrt(dx*dx + dy*dy) of the coordinates (the bits of scipy's pdist), or the matrix a
 *               shortest-path handle kept
 *   u           D[i,k] / r_i, and u = 0 when r_i == 0 (0 / 0 is never evaluated); r_i = radii_host[i]; h = bandwidth
 *   kind        SAFE_WEIGHT_UNIFORM       1.0
 *               SAFE_WEIGHT_TRIANGULAR    max(0, 1 - u)
 *               SAFE_WEIGHT_EPANECHNIKOV  max(0, 1 - u*u)
 *               SAFE_WEIGHT_GAUSSIAN      exp(-0.5 * (t*t)), t = u / h (the argument is exact to the contract; the device's exp
 *                                         is faithfully rounded, not NumPy's bits)
 * A member whose weight is 0 stays a member: the stored pattern is the membership's, with explicit zeros.
 * safe_nbr_weights_from_xy: xy_host f64 [n,2] row-major.  safe_nbr_weights_from_distances: from the kept matrix.  Both take
 * radii_host f64 [n] and build the weights on the device.  Refusals: a non-finite coordinate, a NaN or negative radius, a
 * bandwidth that is not finite and > 0 (read for every kind) SAFE_E_VALUE; no kept distances, an unknown kind, a NULL argument
 * SAFE_E_INVALID.  safe_nbr_set_weights installs the caller's weights, f64 [nnz] in CSR order; a NaN, infinite or negative one
 * is SAFE_E_VALUE.  safe_nbr_weights reads them back in CSR order (SAFE_E_INVALID without weights); safe_nbr_clear_weights
 * removes them.  A refused call leaves the handle's previous weights, or lack of them, as they were.  Synchronous. */
#define SAFE_WEIGHT_UNIFORM 0
#define SAFE_WEIGHT_TRIANGULAR 1
#define SAFE_WEIGHT_EPANECHNIKOV 2
#define SAFE_WEIGHT_GAUSSIAN 3
int safe_nbr_weights_from_xy(safe_nbr *nbr, const double *xy_host, int kind, const double *radii_host, double bandwidth);
int safe_nbr_weights_from_distances(safe_nbr *nbr, int kind, const double *radii_host, double bandwidth);
int safe_nbr_set_weights(safe_nbr *nbr, const double *w_host);
int safe_nbr_weights(safe_nbr *nbr, double *out_host);
int safe_nbr_clear_weights(safe_nbr *nbr);

/* The weighted 'sum' score of columns [col0, col1): ns_dev f64 [n, col1 - col0] row-major,
 *   x_ij = (((0.0 + w_i,k1 * v_k1,j) + w_i,k2 * v_k2,j) + ...)   over the members in ascending k,
 * v = the attribute value widened to f64, NaN -> 0; one accumulator per cell, every product and every sum rounded: this order
 * is the contract.  SAFE_E_INVALID when the handle has no weights.  safe_last_kernel_stats names k_score_weighted (lanes along
 * contiguous columns), or k_permtest_weighted for row-contiguous (Fortran-order) storage: the same sums in the same order. */
int safe_score_weighted(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int64_t col0, int64_t col1, double *ns_dev);

/* safe_moments_test for the weighted score.  Per row, over the members with row_flags = 1 in ascending k: W1_i = sum w,
 * W2_i = sum w*w, c_i their number, and the smallest and the largest w.  With n_v, mu_j, Q_j of safe_attr_column_moments:
 *   g_i = (n_v*W2_i - W1_i*W1_i) / (n_v*(n_v - 1));  var = g_i * Q_j;  z = (x_ij - W1_i*mu_j) / sqrt(var)
 *   g_i := 0 when n_v < 2, or c_i = 0, or c_i = n_v and the smallest flagged weight equals the largest (the whole population
 *   at one weight: decided on min / max, because equal non-dyadic weights leave dust), or the computed value is not positive
 * A cell with var not positive gets pvalues_pos = pvalues_neg = 1 and z = 0.  Tails, nes, nes_binary and the counts are
 * safe_moments_test's.  With all weights 1.0 g_i has the bits of its f_i.  safe_last_kernel_stats names k_weights_emit. */
int safe_moments_test_weighted(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int sign_mode, double enrichment_threshold,
                               int64_t col0, int64_t col1, double *ns_dev, double *pvalues_neg_dev, double *pvalues_pos_dev,
                               double *nes_dev, double *nes_binary_dev, double *num_enriched_dev, double *z_dev /* may be NULL */);

/* safe_permtest_counts for the weighted score ('sum' only): with T_p = row p of the permutation table as safe_perms_read
 * delivers it, S_p[i,j] = the weighted score with v taken at row T_p[k] instead of k, same order;
 * counts_pos = #{p : S_p >= x}, counts_neg = #{p : S_p <= x} as f64 [n, col1 - col0]; ns_dev may be NULL.  Any safe_perms
 * handle.  safe_outputs_from_counts turns the counts into p-values, nes and nes_binary.  safe_last_kernel_stats names
 * k_permtest_weighted. */
int safe_permtest_counts_weighted(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, safe_perms *perms, int64_t col0, int64_t col1,
                                  double *ns_dev, double *counts_neg_dev, double *counts_pos_dev);

/* ---- family-wise adjustment: Westfall-Young single-step max-statistic (maxt.hip) -------------------------------------------
 * Every permutation is a joint draw of all n scores of a column under the null, so the extreme of the standardised scores over
 * a family, per permutation, is the null of the family's extreme whatever the dependence between overlapping neighborhoods.
 * All arithmetic is f64, every operation rounded, in the order written.  Columns j in [col0, col1), rows i, permutations p in
 * [0, P), T_p = row p of the table as safe_perms_read delivers it:
 *   S_p[i,j]    the permuted 'sum' score of safe_permtest_counts_weighted: members added in ascending node order, one
 *               accumulator per cell, NaN -> 0, with the handle's weights if it has some and weight 1.0 otherwise (a flat handle
 *               is accepted: 1.0 * v is exact, the sum is the plain ascending sum)
 *   loc_i, scale_i   k_i and f_i of safe_moments_test on a flat handle, W1_i and g_i of safe_moments_test_weighted (with all its
 *               zeroing rules) on a weighted one; mu_j, Q_j those of safe_attr_column_moments
 *   z_p[i,j]    var = scale_i * Q_j;  z_p = (S_p - loc_i * mu_j) / sqrt(var) when var > 0; otherwise the cell is degenerate,
 *               for every p alike
 *   z_obs[i,j]  the same expression on the observed score: the z_dev of the matching moments entry point, bit for bit, 0 at a
 *               degenerate cell.  live[i,j] = 1 where var > 0, else 0: z_obs = 0 alone does not tell a degenerate cell from a
 *               score that sits on its mean, so the flags travel beside it
 *   tmax[p,j]   the maximum of z_p[i,j] over the non-degenerate i, -inf where there is none; tmin[p,j] the minimum, +inf
 * safe_permtest_extremes: z_dev f64 [n, col1 - col0] and live_dev u8 [n, col1 - col0] row-major (each may be NULL), tmax_dev and
 * tmin_dev f64 [P, col1 - col0] row-major.  Any safe_perms handle.  safe_last_kernel_stats names k_maxt_extremes.
 *
 * safe_counts_from_extremes: z_dev, live_dev [n, m] and tmax_dev, tmin_dev [P, m] as above, complete for all m columns;
 *   scope SAFE_FAMILY_COLUMN   the family is the n neighborhoods of one attribute: E+[p,j] = tmax[p,j], E-[p,j] = tmin[p,j]
 *         SAFE_FAMILY_MATRIX   the family is all n * m cells: E+[p,j] = max over the m columns of tmax[p,.], E- the minimum likewise
 *   counts_pos[i,j] = #{p : E+[p,j] >= z_obs[i,j]},  counts_neg[i,j] = #{p : E-[p,j] <= z_obs[i,j]}  as f64 [n, m];
 *   a degenerate cell gets P in both, the permutation test's own limit (p = 1)
 *   min_counts_neg_dev / min_counts_pos_dev f64 [m] (each may be NULL): the smallest count of column j over its non-degenerate
 *   cells, P if it has none -- divided by P, the attribute's p-value for "enriched somewhere on the network"
 * safe_outputs_from_counts turns the counts into p-values, nes and nes_binary.  safe_last_kernel_stats names k_maxt_counts.
 * Refusals (SAFE_E_INVALID, nothing written): a NULL argument, a bad column range, a table whose row count differs from the
 * membership's, P < 1, an unknown scope.  Both run on the context's stream and return once it has drained. */
#define SAFE_FAMILY_COLUMN 0  /* familywise_scope == 'neighborhoods' */
#define SAFE_FAMILY_MATRIX 1  /* familywise_scope == 'all'           */
int safe_permtest_extremes(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, safe_perms *perms, int64_t col0, int64_t col1,
                           double *z_dev /* may be NULL */, uint8_t *live_dev /* may be NULL */, double *tmax_dev, double *tmin_dev);
int safe_counts_from_extremes(safe_ctx *ctx, int64_t n, int64_t m, int64_t num_permutations, int scope, const double *z_dev,
                              const uint8_t *live_dev, const double *tmax_dev, const double *tmin_dev, double *counts_neg_dev,
                              double *counts_pos_dev, double *min_counts_neg_dev /* may be NULL */,
                              double *min_counts_pos_dev /* may be NULL */);

/* ---- consumers of nes_binary (SAFE.define_top_attributes / define_domains) ---------------- */
/* Connected components of the subgraph induced by the enriched nodes of each candidate
 * attribute (safepy/safe.py:640-655: nx.subgraph + nx.connected_components per attribute).
 * member_host: f64 [n, n_cols] row-major, > 0 = enriched (nes_binary[:, cols]); undirected edges
 * (edge_u[e], edge_v[e]).  labels_host: int32 [n_cols, n]: the smallest node id of the node's
 * component, -1 for nodes that are not enriched. */
int safe_enriched_components(safe_ctx *ctx, int64_t n, int64_t n_edges, const int32_t *edge_u, const int32_t *edge_v,
                             const double *member_host, int64_t n_cols, int32_t *labels_host);
/* scipy.spatial.distance.pdist(x, 'jaccard') as called inside linkage() at safepy/safe.py:673:
 * x_host f64 [m_top, n] row-major (non-zero = set), out_host f64 [m_top (m_top - 1) / 2] in SciPy's
 * condensed order; 0 where both profiles are empty. */
int safe_jaccard_condensed(safe_ctx *ctx, int64_t m_top, int64_t n, const double *x_host, double *out_host);

/* The same two steps on the matrix compute_pvalues left on the device: values_dev is f64 [n, m] row-major (nes_binary), read
 * in place on the context's stream; the chosen columns are host index lists, each index in [0, m) (SAFE_E_INVALID otherwise,
 * nothing written), repeats allowed.  Neither makes a dense copy of the chosen columns.  kernel_ms (may be NULL): the
 * kernels' time, also reported by safe_last_kernel_stats / safe_last_kernel_busy_ms.  Both synchronise.
 *
 * safe_enriched_components_dev: labels_host int32 [n_cols, n] as safe_enriched_components gives them for
 * values[:, cols_host] (> 0 = enriched).  n_cols == 0 writes nothing. */
int safe_enriched_components_dev(safe_ctx *ctx, int64_t n_edges, const int32_t *edge_u, const int32_t *edge_v, const double *values_dev,
                                 int64_t n, int64_t m, const int64_t *cols_host, int64_t n_cols, int32_t *labels_host,
                                 double *kernel_ms);
/* Enriched-pair counts (SAFE.define_top_attributes, attribute_unimodality_metric = 'radius'): for every chosen column a, with
 * E_a = {i : value[i, a] > 0} (NaN, 0, -0.0 and negatives are not enriched),
 *   e_host[a] = |E_a|      q_host[a] = sum over i in E_a, j in E_a of W[i, j]
 * where W is the membership of `within` -- ANY handle: the raw quadratic form, ordered pairs, the diagonal as W holds it; for a
 * symmetric W with a full diagonal (q - e) / 2 is the number of unordered pairs of enriched nodes within reach.  Exact integers:
 * the columns are packed to bits and counted with AND + popcount against the handle's bit matrix.  The host form takes
 * member_host f64 [n, n_cols] row-major with n = the handle's n; the device form reads the columns cols_host (each in [0, m),
 * repeats allowed) of values_dev f64 [n, m] in place on the context's stream, n = the handle's n (SAFE_E_INVALID otherwise),
 * and never copies them densely.  A NULL pointer or a column out of range is SAFE_E_INVALID with nothing written; n_cols == 0
 * writes nothing.  Both synchronise.  safe_last_kernel_stats names k_profile_pack+k_pair_count. */
int safe_enriched_pair_counts(safe_ctx *ctx, safe_nbr *within, const double *member_host, int64_t n_cols, int64_t *q_host,
                              int64_t *e_host);
int safe_enriched_pair_counts_dev(safe_ctx *ctx, safe_nbr *within, const double *values_dev, int64_t n, int64_t m,
                                  const int64_t *cols_host, int64_t n_cols, int64_t *q_host, int64_t *e_host, double *kernel_ms);
/* safe_profile_distances: out_host f64 [m_top (m_top - 1) / 2] = scipy.spatial.distance.pdist(values[:, cols_host].T, metric)
 * (SciPy 1.15, condensed order) for a boolean metric, bit for bit: the columns are packed into bit words (non-zero = set),
 * the four contingency counts of a pair come from popcounts and each metric is one division of exact integers; where a
 * denominator is zero the value is SciPy's (jaccard and yule 0, dice and sokalsneath NaN).  metric: a SAFE_METRIC_* id
 * (SAFE_E_INVALID otherwise).  SAFE_METRIC_JACCARD gives what safe_jaccard_condensed gives.  m_top < 2 writes nothing. */
#define SAFE_METRIC_JACCARD 0
#define SAFE_METRIC_HAMMING 1
#define SAFE_METRIC_DICE 2
#define SAFE_METRIC_ROGERSTANIMOTO 3
#define SAFE_METRIC_RUSSELLRAO 4
#define SAFE_METRIC_SOKALMICHENER 5
#define SAFE_METRIC_SOKALSNEATH 6
#define SAFE_METRIC_YULE 7
int safe_profile_distances(safe_ctx *ctx, const double *values_dev, int64_t n, int64_t m, const int64_t *cols_host, int64_t m_top,
                           int metric, double *out_host, double *kernel_ms);

/* The clustering of define_domains (safepy/safe.py:672-673, linkage(m, method='average', metric=...)) on the device:
 * z_host f64 [m_top - 1, 4] = scipy.cluster.hierarchy.linkage(cond, method='average') of SciPy 1.15, bit for bit, tied
 * distances included (binary profiles give small rationals: ties are the normal case, and the flat clusters fcluster cuts
 * depend on how they are broken).  SciPy's nn_chain is restated step for step -- the chain starts at the smallest live
 * index, a scan keeps the chain predecessor unless another live point is strictly closer and then takes the smallest index
 * of the row minimum, a merge keeps the larger index and averages (nx d_ix + ny d_iy) / (nx + ny) with every operation
 * rounded -- in one persistent workgroup over a square f64 working matrix; the stable sort of the merges by height and the
 * union-find relabel run on the host inside the call.  fcluster stays the caller's (O(m_top) on Z).
 *
 * safe_linkage_average: cond_dev f64 [m_top (m_top - 1) / 2] in SciPy's condensed order, device memory, read on the
 * context's stream and never modified.  safe_profile_linkage: the pack and pair kernels of safe_profile_distances (same
 * arguments, same checks) followed by the linkage, without the condensed vector leaving the device.
 * Both: m_top < 2 writes nothing and returns SAFE_OK.  A distance that is not finite -- NaN or inf from a direct caller;
 * dice / sokalsneath of two empty profiles -- returns SAFE_E_VALUE (SciPy's linkage raises on such input), as does an
 * average that overflows; m_top > SAFE_LINKAGE_MAX_POINTS returns SAFE_E_UNSUPPORTED (the working matrix takes 8 m_top^2
 * bytes, 2 GiB at the limit, and the chain holds 16-bit ids in LDS).  z_host is written only on success.  kernel_ms (may
 * be NULL): the kernels' time, also reported by safe_last_kernel_stats / safe_last_kernel_busy_ms.  Both synchronise. */
#define SAFE_LINKAGE_MAX_POINTS 16384
int safe_linkage_average(safe_ctx *ctx, const double *cond_dev, int64_t m_top, double *z_host, double *kernel_ms);
int safe_profile_linkage(safe_ctx *ctx, const double *values_dev, int64_t n, int64_t m, const int64_t *cols_host, int64_t m_top,
                         int metric, double *z_host, double *kernel_ms);

/* Counts of a whole call -> outputs (safepy/safe.py:528-554 and 468-472): counts_neg / counts_pos are #(S_p <= S_obs) /
 * #(S_p >= S_obs) as f64 [n, m] on the device (e.g. safe_permtest_counts results summed over the ranks of a
 * permutation-axis split), ns_dev the observed scores (NaN = no test; may be NULL).  Writes p-values, NES
 * (nes_table_host as in safe_randomization), nes_binary [n, m] and num_enriched [m].  Precondition: every count is a
 * whole number in [0, num_permutations] wherever the observed score is not NaN -- SAFE_E_VALUE otherwise (e.g. the
 * sum of ranks that each ran the full num_permutations). */
int safe_outputs_from_counts(safe_ctx *ctx, int64_t n, int64_t m, int64_t num_permutations, int sign_mode,
                             double enrichment_threshold, const double *nes_table_host, const double *counts_neg_dev,
                             const double *counts_pos_dev, const double *ns_dev, double *pvalues_neg_dev, double *pvalues_pos_dev,
                             double *nes_dev, double *nes_binary_dev, double *num_enriched_dev);
/* Multi-GPU exchange in integers (replaces gathering f64 NES blocks for the np.concatenate of
 * safepy/safe.py:1355): after safe_randomization / safe_permtest_counts on the bit-sliced or
 * matrix-core kernel, the raw counters of the call are still resident as
 * u32 [m][n_pad] = (#(S_p < S_obs) << 16 | #(S_p > S_obs)), attribute-major, so that a rank's
 * block is one contiguous slab.  safe_export_packed_counts copies them into dst_dev (NULL: only
 * report sizes); *layout is 0 / 1 for the two position orders, -1 if the last call kept no
 * counters (then exchange the f64 outputs instead).  After an all-gather of the slabs (every
 * rank holds the same membership handle, hence the same layout), safe_nes_from_packed_counts
 * turns [m_total][n_pad] counters into NES f64 [n, m_total] row-major with the arithmetic of
 * safepy/safe.py:532-554. */
int safe_export_packed_counts(safe_ctx *ctx, uint32_t *dst_dev, int64_t capacity, int64_t *n_pad, int64_t *m,
                              int *layout);
int safe_nes_from_packed_counts(safe_ctx *ctx, safe_nbr *nbr, const uint32_t *counts_dev, int layout, int64_t n_pad,
                                int64_t m, int64_t num_permutations, int sign_mode, const double *nes_table_host,
                                double *nes_dev);
/* The same exchange for EVERY matrix the reference's compute_pvalues leaves on the instance from the counters
 * (safepy/safe.py:532-554, 468-472): pvalues_neg, pvalues_pos, nes, nes_binary as f64 [n, m] row-major, any of them NULL =
 * not wanted.  One integer all-gather (4 bytes per node x attribute) then serves all four full matrices on every rank --
 * the "final RCCL all-gather of the p-value matrix" without moving 8-byte doubles or transposing blocks. */
int safe_outputs_from_packed_counts(safe_ctx *ctx, safe_nbr *nbr, const uint32_t *counts_dev, int layout, int64_t n_pad,
                                    int64_t m, int64_t num_permutations, int sign_mode, double enrichment_threshold,
                                    const double *nes_table_host, double *pvalues_neg_dev, double *pvalues_pos_dev,
                                    double *nes_dev, double *nes_binary_dev);
/* The same exchange in COLUMN CHUNKS (np.concatenate(axis=1) of safepy/safe.py:1355 is the one exchange of the reference's
 * sharded run, safe.py:1339-1355), optionally overlapped with the last launches of the permutation kernels.
 * safe_set_exchange_chunks(chunks, cols_per_chunk, cb, user) arms the following safe_randomization calls on this context
 * (chunks = 0: off): chunk k = this block's columns [k * cols_per_chunk, (k + 1) * cols_per_chunk), cols_per_chunk a
 * multiple of 64, 1..8 chunks covering the widest rank's block.  safe_export_packed_chunk(k, dst, capacity, stream) copies
 * chunk k's counters (u32 [columns][n_pad], the layout of safe_export_packed_counts; the rest of `capacity` is zeroed) on
 * `stream` -- after the call from the finished counters, so that every rank takes part in the same collectives whatever
 * kernel form its call took (the caller flags slabs that are not bit-sliced counters).
 * With SAFE_HIP_XCHG_TAIL=<fraction> in the environment and >= 2 chunks, the bit-sliced kernel also runs that last part of
 * the permutations as one launch per column chunk and calls cb(user) on the calling thread once every launch is enqueued --
 * before the call waits for them; safe_export_packed_chunk called from there makes `stream` wait until chunk k's counters
 * are final, so the all-gather of chunk k runs while the later chunks compute.  Off by default: at configs[1] it cost the
 * step more than the exchange it hides.  safe_packed_chunk_info tells what the last call did
 * (*chunks = 0: no column-chunked launches).  safe_outputs_from_packed_slabs derives the requested matrices from n_slabs
 * gathered slabs (slab r: slab_cols[r] columns of counters at slabs_dev + r * slab_stride, written to columns out_col0[r]...
 * of f64 [n, m_total] matrices), on `stream` (NULL: the context's), without waiting.  safe_randomization_plan: the counter
 * layout safe_randomization WOULD leave for this block (0 = bit-sliced kernel; -1 otherwise), so that ranks can settle the
 * form of the exchange in the collective they run before the kernels anyway. */
typedef void (*safe_enqueued_fn)(void *user);
int safe_set_exchange_chunks(safe_ctx *ctx, int chunks, int64_t cols_per_chunk, safe_enqueued_fn on_enqueued, void *user);
int safe_packed_chunk_info(safe_ctx *ctx, int *chunks, int64_t *bounds, int64_t *tail_permutations);
int safe_export_packed_chunk(safe_ctx *ctx, int chunk, uint32_t *dst_dev, int64_t capacity, void *stream);
/* The same slab with the counter pair packed to what the permutation count needs (the concatenated blocks of
 * safepy/safe.py:1355 carry counts of at most num_permutations, safe_extras.py:63-66): for num_permutations <= 1023 a pair is
 * 10 + 10 bits, #(S_p < S_obs) << 10 | #(S_p > S_obs), and two outputs travel in five bytes: positions 2 i (low 20 bits)
 * and 2 i + 1 (high 20 bits) of a column make 40 bits -- a column is n_pad / 2 words (low 32 bits of every 40) followed by
 * n_pad / 2 bytes (the high 8), 5 * n_pad / 8 words per column, 0.625 of the u32 slab.  capacity_words: u32 words at dst_dev
 * (the rest is zeroed).  safe_outputs_from_packed_slabs takes such slabs with SAFE_PACKED_NARROW added to `layout`
 * (slab_stride stays in u32 words).  More than 1023 permutations: use the u32 form. */
#define SAFE_PACKED_NARROW 16
int safe_export_packed_chunk_narrow(safe_ctx *ctx, int chunk, uint32_t *dst_dev, int64_t capacity_words, void *stream);
int safe_outputs_from_packed_slabs(safe_ctx *ctx, safe_nbr *nbr, const uint32_t *slabs_dev, int layout, int64_t n_pad, int n_slabs,
                                   int64_t slab_stride, const int64_t *slab_cols, const int64_t *out_col0, int64_t m_total,
                                   int64_t num_permutations, int sign_mode, double enrichment_threshold,
                                   const double *nes_table_host, double *pvalues_neg_dev, double *pvalues_pos_dev,
                                   double *nes_dev, double *nes_binary_dev, void *stream);
int safe_randomization_plan(safe_ctx *ctx, safe_nbr *nbr, safe_attr *attr, int64_t num_permutations, int score_type,
                            int *packed_layout);

/* The exchange step of the attribute-sharded path for hosts without their own collective library
 * (replaces np.concatenate(combined_nes, axis=1), safepy/safe.py:1355, and the process pool around it,
 * safe.py:1339-1353): a thin wrapper over RCCL (ncclAllGather over xGMI), loaded on first use.
 * One rank calls safe_comm_unique_id and hands the SAFE_COMM_ID_BYTES bytes to the others by any means (a
 * file, MPI, a socket); every rank then calls safe_comm_create with its own context (one GPU per rank).
 * safe_allgather_cols enqueues, on the context's stream, the all-gather of every rank's slab of
 * bytes_per_rank bytes at local_dev into all_dev (world_size slabs, rank order) -- e.g. the packed counters of
 * safe_export_packed_counts (attribute-major: a rank's column block IS one slab) or a transposed result
 * block; it returns without waiting (safe_ctx_sync).  SAFE_E_UNSUPPORTED if RCCL cannot be loaded. */
#define SAFE_COMM_ID_BYTES 128
int safe_comm_unique_id(char *id_out, size_t id_len);
int safe_comm_create(safe_ctx *ctx, int world_size, int rank, const char *id, size_t id_len, safe_comm **out);
int safe_comm_destroy(safe_comm *comm);
int safe_allgather_cols(safe_comm *comm, const void *local_dev, size_t bytes_per_rank, void *all_dev);

/* Number of i8 slices the last matrix-core permutation test ran with (2 / 4 / 6: the bits its columns need
 * on their fixed-point grid; 0 if that kernel has not run) -- for roofline reporting. */
int safe_last_mfma_slices(safe_ctx *ctx, int *slices);
/* The filtered form of that kernel (six-slice columns of 'sum' scores, np.dot of safepy/safe_extras.py:15 inside the
 * loop of :56-66): *core_slices = slices the matrix cores multiplied (3 when the filter ran: only the high digits; the
 * compares they cannot decide are settled exactly from the low digits), *undecided = how many compares that was
 * (negative: their list overflowed and the call was repeated with all six slices).  Counts are identical either way. */
int safe_last_mfma_filter(safe_ctx *ctx, int *core_slices, int64_t *undecided);
/* Diagnostics (bench.py's per-step probe): the number of hipMalloc / hipHostMalloc calls the library has made in this process.
 * Buffers are cached per context and per handle shape, so a repeated call of the same shape is expected to add none
 * (the reference allocates every [N, M] temporary anew on each pass: safe_extras.py:50-66). */
int safe_alloc_count(int64_t *calls);
/* Diagnostics: the device blocks the library holds in this process right now -- every hipMalloc it has made whose hipFree it has
 * not (safe_dev_alloc / safe_dev_free included; pinned host memory is not counted).  A call that returns no handle leaves the
 * count as it found it once the context's scratch and pooled blocks have grown to the call's shape; creating and destroying a
 * handle does too.  Unlike hipMemGetInfo the count sees nothing of other processes on the device.  safe_dev_free counts down
 * for whatever pointer it is given: handing it memory that did not come from safe_dev_alloc skews the count. */
int safe_live_alloc_count(int64_t *blocks);
/* Host placement of the seeded stream's sequential part (np.random.seed / np.random.permutation, safepy/safe_extras.py:46,58):
 * the CPUs the library's draw threads may run on (count = 0: wherever the process may).  For LAUNCHERS that place their own
 * threads (bench.py, run_batch): keeping the draw thread off the hardware threads that share a core with the launcher's
 * polling thread.  Applies to draw threads started after the call (one persistent thread per context, created at the
 * first seeded call).  The library never re-pins its caller's threads. */
int safe_set_draw_cpus(const int *cpus, int count);

/* The node table of print_output_files without domains (safepy/safe.py:1297-1306: DataFrame(nes) with key / label columns,
 * to_csv(sep='\t')): rows [r0, r1) of the row-major [n, m] f64 matrix values_dev as the bytes pandas writes, appended to
 * the open file descriptor fd.  Row r is its prefix -- prefix_host[prefix_off_host[r - r0] .. prefix_off_host[r - r0 + 1]),
 * the index / key / label fields as pandas writes them, without the trailing separator -- then '\t' + text(v) per value,
 * then '\n'.  text(v) is NumPy's astype(str) (= repr(float)): the shortest round-trip digits, positional for decimal
 * exponents -4 .. 15, "inf" / "-inf", "-0.0"; NaN gives an empty field (na_rep='').  The text is made on the device in
 * row chunks of at most budget_bytes (bounded by 25 bytes per value; at least one row per chunk) and written through two
 * pinned buffers, chunk c to the file while chunk c + 1 is formatted.  stats_out (may be NULL): double[5] = {format
 * kernels ms, device-to-host copies ms, file writes ms, whole call ms, bytes written}.  Synchronises. */
int safe_format_tsv(safe_ctx *ctx, const double *values_dev, int64_t n, int64_t m, int64_t r0, int64_t r1, const char *prefix_host,
                    const int64_t *prefix_off_host, int fd, int64_t budget_bytes, double *stats_out);

/* Domain contours of plot_composite_network_contours (safepy/safe.py:822-829): SciPy 1.15's gaussian_kernel_estimate for
 * n_sets two-dimensional point sets in one launch.  Set d is the whitened points pts_host[offsets_host[d] .. offsets_host[d+1])
 * (f64 [., 2] row-major; offsets_host int64 [n_sets + 1], offsets_host[0] == 0, non-decreasing) with weights weights_host
 * [same rows] and norm_host[d]; it is evaluated at its g whitened grid points xi_host[d] (f64 [n_sets, g, 2]) into z_host
 * [n_sets, g]: z[d, j] = sum over points i in ascending order of w[i] * (exp(-|p_i - x_j|^2 / 2) * norm[d]), every operation
 * rounded as SciPy's loop rounds it, exp from the device library.  Sets with too few grid points to fill the device are
 * summed in contiguous point chunks whose sums are added in chunk order; no atomics, so every run gives the same z.
 * kernel_ms (may be NULL): the kernels' time.  Synchronises. */
int safe_kde_grid(safe_ctx *ctx, int64_t n_sets, const int64_t *offsets_host, const double *pts_host, const double *weights_host,
                  const double *norm_host, int64_t g, const double *xi_host, double *z_host, double *kernel_ms);

/* Composite colours of plot_composite_network (safepy/safe.py:883-886, groupby(level='domain', axis=1).sum()): counts_host
 * f64 [n, n_domains] = the row-major [n, m] f64 matrix values_dev (read in place, e.g. the device-resident nes_binary) summed
 * over the columns of each domain; domain_host int32 [m] in [0, n_domains) (SAFE_E_VALUE otherwise).  NaN values are skipped.
 * 1 <= n_domains <= 4096 (one f64 LDS bin per domain; SAFE_E_UNSUPPORTED beyond).  Sums of whole numbers are exact; other
 * values are added in an unspecified order.  kernel_ms (may be NULL): the kernel's time.  Synchronises. */
int safe_domain_counts(safe_ctx *ctx, const double *values_dev, int64_t n, int64_t m, const int32_t *domain_host, int64_t n_domains,
                       double *counts_host, double *kernel_ms);

/* Node-to-domain assignment of define_domains (safepy/safe.py:693-705) in one pass over the two device-resident matrices
 * nes_binary_dev and nes_dev (f64 [n, m] row-major, read in place): domain_host int32 [m] is the domain id of every attribute
 * (0 = none), ids_host int32 [n_ids] the sorted distinct ids (SAFE_E_VALUE when they are not, or when a column's id is not
 * among them).  sums_host f64 [n, n_ids]: safe_domain_counts of nes_binary by id.  primary_host int32 [n]: the id >= 1 with
 * the first maximum of the node's sums, or 0 when that maximum is 0 (or there is no id >= 1).  primary_nes_host f64 [n]:
 * the largest non-NaN nes of the node over the attributes of its primary domain (domain 0 included); NaN when all of them
 * are NaN or no attribute has that id (of -0.0 and +0.0 the larger is +0.0).  1 <= n_ids <= 2048 (SAFE_E_UNSUPPORTED
 * beyond).  kernel_ms (may be NULL): the kernel's time, also reported by safe_last_kernel_busy_ms.  Synchronises. */
int safe_node_domains(safe_ctx *ctx, const double *nes_binary_dev, const double *nes_dev, int64_t n, int64_t m,
                      const int32_t *domain_host, const int32_t *ids_host, int64_t n_ids, double *sums_host, int32_t *primary_host,
                      double *primary_nes_host, double *kernel_ms);

/* The nes / nes_binary columns plot_sample_attributes reads (safepy/safe.py:1081-1187): out_host f64 [n, k] row-major =
 * columns cols_host int64 [k] (each in [0, m)) of the row-major [n, m] f64 device matrix values_dev, without copying the
 * rest of it.  kernel_ms (may be NULL): the kernel's time.  Synchronises. */
int safe_gather_columns(safe_ctx *ctx, const double *values_dev, int64_t n, int64_t m, const int64_t *cols_host, int64_t k,
                        double *out_host, double *kernel_ms);

/* The enriched (node, attribute) pairs of a device-resident result matrix as the three arrays of a scipy.sparse CSR or CSC
 * matrix, compacted on the device: what np.nonzero(nes_binary) and nes[rows, cols] give on the host after both [n, m] matrices
 * have been read (the selection of safepy/safe.py:468-472), without moving the other cells across the link.
 *
 * safe_pairs_create (safepy/safe.py:470, the comparison): selector_dev is a row-major f64 [n, m] device matrix, read in place.
 * A cell x is selected when   mode 0: x > 0   mode 1: |x| > threshold   mode 2: x > threshold   mode 3: x < -threshold.
 * The comparison is strict, NaN is never selected, -0.0 is not selected at threshold 0, +-inf are.  The threshold is a number
 * >= 0 or +inf (SAFE_E_VALUE for NaN or a negative one; mode 0 ignores it).  axis 0 counts the selected cells per row (CSR),
 * axis 1 per column (CSC); the counts are scanned on the device and the handle keeps the pointer array (and, for axis 1, the
 * offsets of every 64-row block inside its column) there.  *nnz = the number of selected cells.  kernel_ms (may be NULL):
 * the count and scan kernels' time, also reported by safe_last_kernel_stats.  Synchronises (nnz is a host output).
 * SAFE_E_INVALID: a NULL or negative argument, a mode outside 0..3, an axis outside 0..1.  SAFE_E_UNSUPPORTED, the number in
 * the message: n or m >= 2^31, or nnz >= 2^31 (the indices are int32, what SciPy picks below that).  n == 0 or m == 0 gives
 * an empty selection without a launch (selector_dev may then be NULL).  A refusal leaves *nnz alone and *out NULL.
 *
 * safe_pairs_read (safepy/safe.py:470-472, the cells the comparison picked): evaluates the same comparison over
 * selector_dev once more and writes indptr_host int32 [n + 1] (axis 0) or [m + 1] (axis 1), indices_host int32 [nnz] -- the
 * column indices of every row in ascending order, or the row indices of every column in ascending order -- and data_host
 * f64 [nnz]: the cells of values_dev (row-major f64 [n, m] on the device; may be selector_dev itself) at those places, copied
 * bit for bit (NaN payloads, signed zeros, denormals).  values_dev NULL: the pattern only, data_host is not touched and may be
 * NULL.  Indices and values are gathered into device buffers of the call and copied out; it has host outputs, so it
 * synchronises.  May be called again (other values).  kernel_ms (may be NULL): the emit kernel's time.
 * selector_dev is the caller's memory and must hold what safe_pairs_create saw.  If it does not, nothing is stored outside
 * the range the scan gave each row or column, and the call fails with SAFE_E_VALUE ("selection changed between create and
 * read").  A refusal writes nothing to indptr_host, indices_host or data_host.
 *
 * safe_pairs_destroy waits for the context's stream and frees the handle's device arrays.  NULL is fine. */
int safe_pairs_create(safe_ctx *ctx, const double *selector_dev, int64_t n, int64_t m, int mode, double threshold, int axis,
                      safe_pairs **out, int64_t *nnz, double *kernel_ms);
int safe_pairs_read(safe_pairs *pairs, const double *selector_dev, const double *values_dev, int32_t *indptr_host,
                    int32_t *indices_host, double *data_host, double *kernel_ms);
int safe_pairs_destroy(safe_pairs *pairs);

/* Additive: the gene-to-term matrix of safepy/utils/make_go.py (make_locus2term, :247-289) built on the device from the
 * direct annotations and the is_a DAG of one branch: "a matrix of gene-to-term annotations (propagated)" (:18-26).
 * Cell (row, term) = 1 iff the row (a locus) is annotated to the term or to any descendant of it -- the full ancestor
 * closure, where the reference's store_predecessors_all (:206-229) keeps one path per term.  Then terms
 * without a row are dropped (:273-275), then every row without a term that missing_rows does not flag is given to the
 * root (:277-280), whose column stays in its place among the terms.
 *
 * safe_go_create: child_ptr int32 [n_terms + 1] / child_idx int32 [child_ptr[n_terms]]: the children of every term (CSR);
 * ann_row / ann_term int32 [n_ann]: the direct annotations, duplicates allowed; root: the term that takes the rows
 * without one; missing_rows u8 [n_rows] or NULL: rows the annotations do not know (they stay empty, are not given to
 * the root, and are NaN in safe_go_as_attr).  All host memory.  The library levels the terms itself (leaves are level
 * 0, any other term 1 + the maximum over its children) and runs one launch per level on the context's stream; scratch
 * comes from the context.  Outputs: *n_kept = terms with at least one row, *nnz = ones of the matrix,
 * *num_root_assigned = rows given to the root (the number the reference prints, :284); kernel_ms (may be NULL): the
 * six passes' time.  Synchronises (the totals are host outputs).
 * SAFE_E_VALUE, before anything is allocated or launched: a cycle among the edges; an index out of range (child, root,
 * annotation row or term); an annotation on a row of missing_rows; n_rows / n_terms / n_ann that are not below 2^31 (or
 * n_rows, n_terms below 1).  SAFE_E_UNSUPPORTED: nnz >= 2^31, or more cells than one launch covers.  A refusal writes
 * to none of the output pointers.
 *
 * safe_go_read: indptr_host int64 [n_kept + 1], indices_host int32 [nnz] (the rows of every kept term, ascending),
 * kept_host int32 [n_kept] (the indices of the kept terms, ascending); *num_root_assigned may be NULL.  The same input
 * gives the same bytes.  safe_go_as_attr: the CSC expanded, on the device, into the f32 [n_rows, n_kept] safe_attr that
 * safe_attr_create_csc_host makes of the arrays safe_go_read returns (NaN across missing_rows); the handle may be
 * destroyed afterwards.  safe_go_pass_ms: ms [SAFE_GO_PASSES] of the create call -- zero + scatter, closure, counts,
 * root, scans, emit -- and the number of levels (may be NULL).  safe_go_destroy waits for the context's stream; NULL is fine. */
#define SAFE_GO_PASSES 6
int safe_go_create(safe_ctx *ctx, int64_t n_rows, int64_t n_terms, const int32_t *child_ptr, const int32_t *child_idx, int64_t n_ann,
                   const int32_t *ann_row, const int32_t *ann_term, int64_t root, const uint8_t *missing_rows, safe_go **out,
                   int64_t *n_kept, int64_t *nnz, int64_t *num_root_assigned, double *kernel_ms);
int safe_go_read(safe_go *go, int64_t *indptr_host, int32_t *indices_host, int32_t *kept_host, int64_t *num_root_assigned);
int safe_go_as_attr(safe_go *go, safe_attr **out);
int safe_go_pass_ms(safe_go *go, double *ms, int64_t *n_levels);
int safe_go_destroy(safe_go *go);

/* Name and average duration (ms) of the dominant kernel of the last enrichment call,
 * measured with HIP events on the context stream (bench.py's roofline object). */
int safe_last_kernel_stats(safe_ctx *ctx, char *name, size_t name_len, double *avg_ms,
                           int64_t *launches);

/* Time (ms) during which at least one launch of that kernel was running in the last enrichment call: the union of the launches'
 * intervals.  Consecutive launches of the permutation kernels run on two streams and overlap, so launches x avg_ms exceeds it
 * (and can exceed the call).  Measurement only; no reference counterpart. */
int safe_last_kernel_busy_ms(safe_ctx *ctx, double *busy_ms);

#ifdef __cplusplus
}
#endif
#endif /* SAFE_HIP_H */
