/* ghf.h — C ABI of libghf_hip.so: the MI355X (gfx950) HyperGNN forward hot path.
 *
 * The reference (danieleschmidt/Graph-Hypernetwork-Forge v0.2.0) has no FFI or
 * plugin interface; its boundary for this path is two nn.Module call signatures
 * (SURVEY.md §8b).  Each entry point below replaces a span of stock ATen CPU ops
 * inside those two calls; the span is cited as reference file:line (paths
 * relative to graph_hypernetwork_forge/).  The Python host mirror that binds
 * these with ctypes is graph-hypernetwork-forge_amd/_native.py; INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - Plain pointers and sizes only; every pointer is DEVICE memory owned by the
 *    caller (torch's caching allocator in the Python host).  Inputs are never
 *    written.  Nothing is allocated, freed or synchronised inside any call.
 *  - Every call enqueues on `stream` (a hipStream_t passed as void*) and returns
 *    immediately; calls are re-entrant and graph-capturable.
 *  - Return 0 on success, a negative GHF_E* code otherwise; ghf_last_error()
 *    gives a thread-local message.
 *  - All floating point is IEEE fp32; indices are int64 at the API (as in
 *    models/hypergnn.py:191) and int32/uint32 inside a plan.
 */
#ifndef GHF_H
#define GHF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GHF_ABI_VERSION 15

#define GHF_OK            0
#define GHF_EINVAL       -1   /* bad argument (shape, alignment, unsupported size) */
#define GHF_EHIP         -2   /* a HIP runtime call failed */
#define GHF_EUNSUPPORTED -3   /* no kernel for this configuration */

/* ghf_message_layer_fwd flags */
#define GHF_FLAG_NO_TAIL  1   /* write sum_e(...) / max(indeg,1) only: skip residual+ReLU+LayerNorm */
#define GHF_FLAG_RAW_SUM  2   /* (implies NO_TAIL) write sum_e(...) itself, no division: the backward passes */
#define GHF_FLAG_ZERO_SRC 4   /* the kernel MUST leave the source half of every relation's weights (W_msg) out: no source-row
                                 gathers, no products with that half — whatever the packed tensor holds there (the backward
                                 hands ONE packed [W_msg^T; W_self^T] to both of its gradient passes and names the half each
                                 pass must not read; a half that really is zero gives the same result without the flag).
                                 Honoured by the kernels with the side output (ghf_message_side_output_supported) only:
                                 elsewhere the call returns GHF_EUNSUPPORTED — pack that half as zeros and drop the flag */
#define GHF_FLAG_ZERO_DST 8   /* the same for the destination half (W_self); not both */
#define GHF_FLAG_ADD_H   16   /* with NO_TAIL / RAW_SUM: h_out = (that result) + h — `h` then only names the rows to add (the gathers use
                                 h_split): the backward accumulates its gradient terms this way.  Kernels with the side
                                 output (ghf_message_side_output_supported) only */

/* Weight layouts produced by ghf_weightgen_fwd and consumed by ghf_message_layer_fwd */
#define GHF_WLAYOUT_NATURAL 0 /* W_msg[R][d_in][d_out], W_self[R][d_in][d_out] row-major, as the reference returns them */
#define GHF_WLAYOUT_FRAG16  1 /* MFMA 16x16x4 B-fragment order: Wfrag[R][d/16][2d/16][64 lanes][4] */
/*      (2: three exact bf16 pieces — retired with its kernel in ABI 10; the number is not reused) */
#define GHF_WLAYOUT_SPLIT2H 3 /* fp16 MFMA 16x16x32 B-fragment order, every weight of relation r scaled by a power of two
                                 2^s(r) and cut into 2 fp16 pieces: Wh[R][d/16][2d/32][2 pieces][64 lanes][8] fp16 = 4 bytes
                                 per weight, followed by float 2^-s(r) [R] */

int         ghf_abi_version(void);
const char* ghf_last_error(void);

/* HOST function (no device work, no stream): a position-dependent 64-bit checksum of `nbytes` bytes (a multiple of 8) at `p`.
 * The plan cache confirms a hit on a long relation list with it: the list's array of object pointers against the checksums
 * taken when the plan was built — the per-call string -> id mapping of models/hypergnn.py:264-268 at memory speed. */
unsigned long long ghf_host_checksum64(const void* p, size_t nbytes, unsigned long long seed);
/* HOST function: dense ids of an array of `n` machine words (a relation list's object pointers) in first-appearance order —
 * ids[i] (int64, what ghf_plan_build takes) = the rank of words[i] among the distinct words by first appearance, uniq[k] = the
 * k-th distinct word.  Returns the number of distinct words, or -1 when there are more than max_uniq (the caller then falls
 * back to hashing the strings).  `threads` > 1: the array beyond a prefix is mapped by that many host threads (same result).
 * The reference's dict.fromkeys pass (models/hypergnn.py:264-268) for lists that reference a few string objects many times. */
long long ghf_host_word_ids(const void* words, long long n, long long* ids, void** uniq, long long max_uniq, int threads);

/* Which plan geometry and weight layout the message kernel for hidden size d wants.
 * block_nodes == 1 means "CSR by destination" (the generic kernel; chunk_rows == split_chunks == 0 then). */
int ghf_message_config(int d, int* block_nodes, int* wlayout, int* chunk_rows, int* split_chunks);

/* ---- K0: graph plan -----------------------------------------------------------
 * Replaces the implicit edge order of models/hypergnn.py:191 (src,dst = edge_index)
 * and the in-degree count of :207-212.  Sorts edges by (dst / block_nodes, rel,
 * dst % block_nodes), i.e. key = (dst/BN)*R*BN + rel*BN + dst%BN, and emits
 *   sorted_key [E] uint32,
 *   sorted_src [E] int32: the source node id; for BN > 1 bits 28..31 also hold the edge's
 *              "run head": with t = (position in its (block, relation) group) % 16, the
 *              smallest t' <= t such that positions t'..t of that 16-row tile all have the
 *              same destination (needs N <= 2^28),
 *   seg_off [nseg+1] int32 with nseg = ceil(N/BN)*R  (BN > 1)  or  N  (BN == 1: CSR rows),
 *   indeg [N] int32,
 *   chunk_tab [2*max_chunks] int32 and blk_chunk_off [ceil(N/BN)+1] int32 (BN > 1 only, else
 *              NULL): every (block, relation) group cut into chunks of <= chunk_rows edges;
 *              chunk c = { first sorted edge, (rel << 8) | (cross << 7) | rows }, cross = a run of
 *              equal destinations spans a 16-row tile boundary inside the chunk; block b owns
 *              chunks [blk_chunk_off[b], blk_chunk_off[b+1]),
 *   item_tab [4*max_items] int32 and blk_item_off [ceil(N/BN)+1] int32 (BN > 1 only): the work items.
 *              A block is one item, or several for one of two reasons.  A block with more than split_chunks
 *              chunks (the hub of a power-law graph) is cut into ceil(chunks/split_chunks) items.  And the blocks
 *              of the last, partly filled round of workgroups: with NB = ceil(N/BN) blocks on the current device's
 *              C compute units and rem = NB % C, when NB > C and 0 < 2*rem <= C each of the blocks NB-rem .. NB-1
 *              becomes min(8, C / rem, chunks / 8) items (integer divisions: at least 8 chunks per item) where
 *              that is more than the hub rule gives it — so the item count of a plan depends on the compute-unit
 *              count of the device it was built on.  k items cut a block's n chunks evenly: per = ceil(n / k),
 *              item j = chunks [j*per, min((j+1)*per, n)), none of them empty.  Item i = { block, first chunk,
 *              one past its last chunk, scratch slot }: the items of blocks with several take the slots 0, 1, ..
 *              in item order, the only item of a block has slot -1; block b owns items
 *              [blk_item_off[b], blk_item_off[b+1]),
 *   status [3] int32: [0] 0 ok, bit0 = a src/dst outside [0,N), bit1 = a rel outside [0,R) (read it back
 *              before trusting the plan; offending edges are dropped); [1] number of items; [2] number of
 *              scratch slots (each BN*d floats) ghf_message_layer_fwd needs in `partial`.
 * Requires ceil(N/BN)*BN*R < 2^32, E < 2^31, R < 2^23, chunk_rows % 4 == 0 (% 16 for the kernels that read the run heads), chunk_rows < 128, split_chunks > 0. */
size_t  ghf_plan_workspace_bytes(int64_t N, int64_t E, int R, int block_nodes, int chunk_rows);
int64_t ghf_plan_max_chunks(int64_t N, int64_t E, int R, int block_nodes, int chunk_rows);
int64_t ghf_plan_max_items(int64_t N, int64_t E, int R, int block_nodes, int chunk_rows, int split_chunks);
int ghf_plan_build(const int64_t* edge_index /* [2,E] row 0 = src, row 1 = dst */,
                   const int64_t* rel_id /* [E] */, int64_t N, int64_t E, int R, int block_nodes,
                   int chunk_rows, int split_chunks, void* workspace, size_t workspace_bytes,
                   uint32_t* sorted_key, int32_t* sorted_src, int32_t* seg_off, int32_t* indeg,
                   int32_t* chunk_tab, int32_t* blk_chunk_off, int32_t* item_tab, int32_t* blk_item_off,
                   int32_t* status, void* stream);

/* ---- node-batch subgraph: the k-hop in-neighbourhood of a seed list (HyperGNN.forward_nodes) -------------------
 * No counterpart in the reference: a k-layer HyperGNN row depends only on the rows within k hops upstream of it
 * (models/hypergnn.py:190-230, 288-296: a mean over the row's in-edges, a self term, a residual and a LayerNorm of that
 * row), so the rows of a batch of seeds can be computed on that subgraph alone.  All three calls read the edges of a plan of
 * ghf_plan_build (sorted_key / sorted_src [E], N, R, block_nodes as built), decoded as its comment above says: block plans
 * (block_nodes > 1) carry the source in bits 0..27 of sorted_src, CSR plans the whole word.  Integer arithmetic only; no
 * result depends on the order in which the device runs the work.  One caller-allocated workspace serves all three:
 *   ghf_subgraph_workspace_bytes: its size (256-byte aligned), 0 for bad sizes.
 *   ghf_subgraph_hops:  dist [N] int32: dist[v] = the fewest edges u -> v on a path from v to a seed, k + 1 where that
 *                       exceeds k.  seeds [S] int64: duplicates allowed; ids outside [0, N) are skipped (validate them
 *                       first).  At most k passes over the edges; once a pass discovers nothing the later ones return at
 *                       once (a word of the workspace: no host sync).
 *   ghf_subgraph_nodes: from dist: node_list [N] int64, whose first m[k] entries are the nodes with dist <= k ordered by
 *                       (dist, node id) (the rest is not written); new_id [N] int64: v's position in node_list, -1 beyond
 *                       k hops; m [k+1] int64: m[j] = the number of nodes with dist <= j — they are the first m[j] entries.
 *                       It is not told E and uses the head of the shared workspace only: what it requires, and refuses to
 *                       run below, is ghf_subgraph_workspace_bytes(N, 0, k).
 *   ghf_subgraph_edges: the edges whose destination has dist <= k - 1 (their sources have dist <= k), in the plan's sorted
 *                       order (a stable compaction): edge_out [2, E] int64 (row stride E): edge_out[p] = new_id[src],
 *                       edge_out[E + p] = new_id[dst]; rel_out [E] int64: the relation id, p < E'; num_edges [1] int64 = E'.
 * Requires 0 < N < 2^31 - 1, 0 <= E < 2^31 - 1, k >= 1 and the plan's ceil(N/BN)*BN*R < 2^32. */
size_t ghf_subgraph_workspace_bytes(int64_t N, int64_t E, int k);
int ghf_subgraph_hops(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                      const int64_t* seeds, int64_t S, int k, void* workspace, size_t workspace_bytes, int32_t* dist,
                      void* stream);
int ghf_subgraph_nodes(const int32_t* dist, int64_t N, int k, void* workspace, size_t workspace_bytes, int64_t* node_list,
                       int64_t* new_id, int64_t* m /* [k+1] */, void* stream);
int ghf_subgraph_edges(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                       const int32_t* dist, const int64_t* new_id, int k, void* workspace, size_t workspace_bytes,
                       int64_t* edge_out /* [2, E] */, int64_t* rel_out /* [E] */, int64_t* num_edges /* [1] */, void* stream);

/* ---- sampled node-batch subgraph: per-hop fanout caps (HyperGNN.forward_nodes(..., fanout, seed)) ------------------
 * The layer aggregates by mean, so a uniform sample without replacement of a row's in-edges is an unbiased estimate of that
 * row's aggregate.  Inputs: fanout [k] (HOST array of ints, each -1 or >= 1) and a 64-bit seed.  Hop j (0 <= j < k) expands
 * the nodes first reached at sampled distance j (the seeds are distance 0).  For such a node t:
 *   fanout[j] == -1, or t has at most fanout[j] in-edges: every in-edge of t is kept;
 *   otherwise exactly fanout[j] are kept: those with the smallest (priority(e), position(e)).
 * position(e) is the edge's index in the plan's sorted order (its index in sorted_key / sorted_src) and, in uint64
 * arithmetic modulo 2^64 (splitmix64: Steele, Lea & Flood 2014, with Vigna's constants),
 *   z = seed + (position(e) + 1) * 0x9E3779B97F4A7C15
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *   z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *   z =  z ^ (z >> 31)
 *   priority(e) = z >> 32                                   (a 32-bit integer)
 * Sources of kept edges that have no distance yet get distance j + 1.  A node is expanded once, at the hop that first
 * reached it; nodes at distance k are not expanded; parallel edges are separate edges.  So every destination at distance
 * j <= k - 1 has at most fanout[j] kept in-edges, their sources are at distance <= j + 1, and node_list ordered by
 * (dist, id) keeps the "rows within j hops are a prefix" property.  The result is a pure function of (plan, seeds, fanout,
 * seed): no value written depends on which thread lands first.  It depends on the PLAN's order: plans of the same graph
 * with another geometry (hidden size, recorded or not) number the edges differently, and the same seed then picks other
 * edges.  With every fanout[j] == -1 or >= the largest in-degree the outputs equal ghf_subgraph_*'s bit for bit.
 *   ghf_subgraph_sample_workspace_bytes: the workspace of the three stages (256-byte aligned), 0 for bad sizes: the scan
 *                       arrays of ghf_subgraph_workspace_bytes plus, per edge, two 64-bit sort keys and two 32-bit values.
 *   ghf_subgraph_sample_hops: dist [N] int32 (sampled distance, k + 1 when not reached) and keep [E] int32 (1: the edge at
 *                       that plan position is kept).  A capped hop: flags, a scan, a compaction into keys (dst << 32 |
 *                       priority) with the position as value, one stable radix sort, one selection pass; a hop with
 *                       fanout -1: one pass over the edges, no sort.  UNLIKE every other call, a capped hop reads ONE word
 *                       back on the host (the number of candidate edges: the sort's length) and waits for `stream`: the call
 *                       is not graph-capturable.  At most k reads, none for a hop with fanout -1; the first capped hop that
 *                       reads a count of zero ends the stage (the later hops are skipped).  The host does not learn of an
 *                       uncapped hop that reached nobody before the next capped hop's read.  host_reads (HOST pointer, may
 *                       be NULL) receives their number.
 *   ghf_subgraph_nodes: as above, on dist, with this workspace.
 *   ghf_subgraph_sample_edges: the kept edges in the plan's sorted order (a stable compaction), renumbered by new_id, with
 *                       the plan's relation ids: edge_out / rel_out / num_edges as ghf_subgraph_edges.
 * Requires what ghf_subgraph_* requires. */
size_t ghf_subgraph_sample_workspace_bytes(int64_t N, int64_t E, int k);
int ghf_subgraph_sample_hops(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                             const int64_t* seeds, int64_t S, int k, const int* fanout /* HOST [k] */, uint64_t seed,
                             void* workspace, size_t workspace_bytes, int32_t* dist, int32_t* keep /* [E] */,
                             int64_t* host_reads /* HOST [1] or NULL */, void* stream);
int ghf_subgraph_sample_edges(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                              const int32_t* keep, const int64_t* new_id, void* workspace, size_t workspace_bytes,
                              int64_t* edge_out /* [2, E] */, int64_t* rel_out /* [E] */, int64_t* num_edges /* [1] */, void* stream);

/* ---- node-batch subgraph without given edges (HyperGNN.forward_nodes(..., exclude=)) -----------------------------
 * Link prediction trains on batches of edges (head, relation, tail) that the model is asked to score; the subgraph the
 * rows are computed on must not contain them (PyG's LinkNeighborLoader, DGL's as_edge_prediction_sampler(exclude=...)).
 * An exclusion set X is a list of pairs (s, t) (typed == 0) or triples (s, t, r) (typed == 1).  An edge u -> v with
 * relation id p of the plan is EXCLUDED iff (u, v) is in X (untyped) or (u, v, p) is in X (typed):
 *   every parallel edge that matches is excluded; direction matters ((t, s) is another entry: callers who want the
 *   reverses list them); entries that match no edge do nothing; duplicates change nothing.
 * Excluded edges do not exist for the call: no hop walks them, they are not emitted, so they count in no in-degree of the
 * plan built from the emitted edges, and in the sampled form they are not candidates — a destination with f + 1 in-edges
 * of which one is excluded keeps the remaining f under cap f.  priority(e) stays a function of the edge's position in the
 * FULL plan, as defined above.  So the outputs are those of the twin call on a plan of the graph without the excluded
 * edges, except that the sampled draw numbers the edges by the full plan.
 * Key encoding: excl [n_excl] uint64 on the device, SORTED ASCENDING by the caller (as the filter lists of ghf_score_rank):
 *   untyped: (uint64)s << 32 | t
 *   typed:   (uint64)s << 32 | (t * R + r)          (t * R + r < 2^32: every plan requires ceil(N/BN)*BN*R < 2^32)
 * An unsorted list may miss matches but never faults: the binary search stays inside [0, n_excl), and node and relation
 * ids are compared as numbers, never used as indices, so no entry needs to be in range.
 * The list is probed only for an edge that would otherwise be taken — a hop: destination at distance j and source
 * unvisited; the edges stage: destination within k - 1 hops; the sampled hop: a candidate (flag pass, or the uncapped
 * pass) — so the probes follow the subgraph's size, not E * log n.  Whether an edge is excluded is a function of the edge
 * alone: the results stay independent of which thread lands first.
 *   ghf_subgraph_hops_excl, ghf_subgraph_edges_excl, ghf_subgraph_sample_hops_excl: their twins' arguments, then excl,
 *                       n_excl, typed.  The same workspaces (ghf_subgraph_workspace_bytes / _sample_workspace_bytes): there
 *                       is no per-edge array of excluded edges.  With n_excl == 0 (excl may be NULL) they equal their twins
 *                       bit for bit.  n_excl < 0, excl == NULL with n_excl > 0, and typed other than 0 or 1 are GHF_EINVAL,
 *                       checked on the host before any other argument is looked at.
 *   ghf_subgraph_nodes and ghf_subgraph_sample_edges serve unchanged: dist has no distance through an excluded edge, and
 *                       keep[] never marks one. */
int ghf_subgraph_hops_excl(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                           const int64_t* seeds, int64_t S, int k, void* workspace, size_t workspace_bytes, int32_t* dist,
                           void* stream, const uint64_t* excl /* [n_excl] ascending */, int64_t n_excl, int typed);
int ghf_subgraph_edges_excl(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                            const int32_t* dist, const int64_t* new_id, int k, void* workspace, size_t workspace_bytes,
                            int64_t* edge_out /* [2, E] */, int64_t* rel_out /* [E] */, int64_t* num_edges /* [1] */,
                            void* stream, const uint64_t* excl /* [n_excl] ascending */, int64_t n_excl, int typed);
int ghf_subgraph_sample_hops_excl(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R,
                                  int block_nodes, const int64_t* seeds, int64_t S, int k, const int* fanout /* HOST [k] */,
                                  uint64_t seed, void* workspace, size_t workspace_bytes, int32_t* dist,
                                  int32_t* keep /* [E] */, int64_t* host_reads /* HOST [1] or NULL */, void* stream,
                                  const uint64_t* excl /* [n_excl] ascending */, int64_t n_excl, int typed);

/* ---- K1: weight generation ------------------------------------------------------
 * Replaces models/weight_generator.py:137-141 (three nn.Sequential heads, reshape,
 * * exp(log_scale)) for B = R relation embeddings at once.
 *  head_params: 3 heads (W_msg, W_self, bias) x (num_hidden+1) Linear layers x {weight,bias},
 *               flattened as head_params[(head*(num_hidden+1) + layer)*2 + {0,1}];
 *               weights are [out,in] row-major as nn.Linear stores them.
 *  log_scales: host array of three device pointers, one float each (the reference's three 1-element parameters
 *               log_scales.{W_msg,W_self,bias}, weight_generator.py:85-88, read in place).
 *  hidden_ws:   scratch for hidden activations, >= 3*2*R*max(Hh,T) floats.
 *  layout NATURAL: W_msg,W_self [R,d_in,d_out], bias [R,d_out] (any d_in,d_out).
 *  layout FRAG16:  requires d_in == d_out == d, d % 16 == 0; W_msg is the combined
 *                  fragment buffer of 2*R*d*d floats and W_self must be NULL.
 *  hidden_drop:    training with dropout > 0 (the reference's Linear -> ReLU -> Dropout, weight_generator.py:96-107): the masks,
 *                  already scaled by 1/(1-p), as floats [3 heads][num_hidden][R][Hh] (ghf_weightgen_acts' layout), multiplied
 *                  into every hidden activation; NULL: none.  The caller draws them (the reference draws them with torch's
 *                  generator; so does the Python mirror).
 *  acts:           NULL, or where the same launch leaves every hidden layer's output (ghf_weightgen_acts' result and layout:
 *                  what the backward needs besides the outputs). */
int ghf_weightgen_fwd(const float* text_emb /* [R,T] */, const float* const* head_params,
                      const float* const* log_scales /* [3] host array of device pointers */, int R, int T, int Hh, int num_hidden,
                      int d_in, int d_out, int layout, float* hidden_ws,
                      float* W_msg, float* W_self, float* bias, const float* hidden_drop /* or NULL */, float* acts /* or NULL */,
                      void* stream);

/* The L generators of one model (identical shapes: the reference builds one WeightGenerator per layer, hypergnn.py:131-143) in
 * ONE launch sequence — hidden layers, output layers, packing: three kernels for all layers instead of three per layer; on
 * small graphs the generators' launches are a large share of a forward (BASELINE configs 1 and 2).  head_params: generator
 * g's pointers at [g * 3 * (num_hidden + 1) * 2 ...] in ghf_weightgen_fwd's order; log_scales [L * 3]; hidden_ws: L times
 * ghf_weightgen_fwd's size; W_msg / W_self / bias: host arrays of L device pointers (W_self NULL or its entries NULL where
 * the layout has none).  Inference only (no dropout masks).  L <= 8.  Same values as L calls of ghf_weightgen_fwd. */
int ghf_weightgen_fwd_batched(int L, const float* text_emb, const float* const* head_params, const float* const* log_scales,
                              int R, int T, int Hh, int num_hidden, int d_in, int d_out, int layout, float* hidden_ws,
                              float* const* W_msg, float* const* W_self, float* const* bias, void* stream);

/* ---- text encoder ------------------------------------------------------------------
 * Replaces models/hypergnn.py:39-81 (TextEncoder) for U strings at once:
 *   out[u] = tanh( mean_{c < lens[u]} char_emb[ids[u][c]] . W^T + b )
 * ids [U, Lmax] int32 = min(ord(ch), 127) per character, padded ('' is the single id 0: lens[u] >= 1); ids outside
 * [0, V) are clamped.  char_emb [V, C], W [T, C] and b [T] as nn.Embedding / nn.Linear store them. */
int ghf_text_encode_fwd(const int32_t* ids, const int32_t* lens, int U, int Lmax,
                        const float* char_emb, int V, int C, const float* W, const float* b, int T,
                        float* out /* [U,T] */, void* stream);

/* ---- input projection -------------------------------------------------------------
 * Replaces models/hypergnn.py:261: h0 = relu(x @ W_in^T + b_in).  x [N,F], W_in [d,F]. */
int ghf_input_proj_fwd(const float* x, const float* W_in, const float* b_in,
                       int64_t N, int F, int d, float* h0,
                       void* h_split /* optional: the rows of h0 as ghf_split_rows(split_layout) would write them */,
                       int split_layout, void* stream);

/* ---- K2+K3: one message-passing layer ---------------------------------------------
 * Replaces models/hypergnn.py:281-296: per-edge weight gather, h_u @ W_msg[r] + bias[r],
 * mean at targets, mean-W_self self-loop, residual, ReLU, LayerNorm — as
 *   out_v = (1/max(indeg_v,1)) * sum_{e=(u->v)} (h_u W_msg[r_e] + bias[r_e] + h_v W_self[r_e])
 *   h'_v  = LayerNorm(ReLU(out_v + h_v))              
 * for destination rows [row0, row0+rows) (row0 % block_nodes == 0); other rows of
 * h_out are not touched.  The plan arrays must come from ghf_plan_build with the
 * same N, E, R, block_nodes; W/bias from ghf_weightgen_fwd with `wlayout`.
 * item0 / n_items: the work items of the blocks of the row range, i.e. blk_item_off[row0/BN] and
 * blk_item_off[ceil((row0+rows)/BN)] - item0 (host copies of two plan words); partial: scratch of
 * status[2]*BN*d floats for the split blocks (may be NULL when status[2] == 0).
 * h_split: the rows of h cut into pieces by ghf_split_rows (or by a previous call's h_split_out); required when
 * wlayout is SPLIT2H, ignored otherwise.  h_split_out (optional, that layout only, not with
 * GHF_FLAG_NO_TAIL): receives the split form of the h_out rows written by this call, for the next layer.
 * agg_out (optional, not with GHF_FLAG_NO_TAIL; ghf_message_side_output_supported): also receives, for the rows written,
 * the aggregate before the tail — what GHF_FLAG_NO_TAIL would have written to h_out — which a training forward keeps for
 * ghf_tail_bwd (the reference's autograd keeps the same tensor, hypergnn.py:281-296). */
int ghf_message_side_output_supported(int d, int block_nodes, int wlayout);
int ghf_message_layer_fwd(const float* h /* [N,d] */, const void* h_split /* ghf_split_rows output or NULL */, int64_t N, int d,
                          const uint32_t* sorted_key, const int32_t* sorted_src,
                          const int32_t* seg_off, const int32_t* indeg,
                          const int32_t* chunk_tab, const int32_t* blk_chunk_off,
                          const int32_t* item_tab, const int32_t* blk_item_off,
                          int64_t item0, int64_t n_items, float* partial,
                          int64_t E, int R, int block_nodes,
                          const float* W_msg, const float* W_self, const float* bias, int wlayout,
                          const float* ln_gamma, const float* ln_beta, float ln_eps,
                          int64_t row0, int64_t rows, float* h_out /* [N,d] */,
                          void* h_split_out /* or NULL */, float* agg_out /* [N,d] or NULL */, int flags, void* stream);

/* Rows [row0, row0+rows) of h [N,d] in the form the message kernel of `wlayout` gathers (the split is done once per
 * row here instead of once per edge there); h_split holds ghf_split_rows_bytes(N, d, wlayout) bytes:
 *   SPLIT2H: h_split[v][2 pieces][d] fp16 — x 2^s(v) = hi + lo (22 significand bits), 2^s(v) lifting the row's largest
 *            magnitude into [2^13, 2^14) — followed by float 2^-s(v) [N].
 * Other layouts gather h itself (ghf_split_rows_bytes == 0).  d % 4 == 0. */
size_t ghf_split_rows_bytes(int64_t N, int d, int wlayout);
int ghf_split_rows(const float* h, int64_t N, int d, int64_t row0, int64_t rows, int wlayout, void* h_split, void* stream);

/* Bytes of the W_msg buffer ghf_weightgen_fwd fills in `wlayout` (NATURAL: one of the two [R,d_in,d_out] matrices). */
size_t ghf_weights_bytes(int R, int d_in, int d_out, int wlayout);

/* ---- range guard of the two-fp16-piece forms ------------------------------------------------------------------------
 * GHF_WLAYOUT_SPLIT2H rows and weights keep 22 significand bits of every element within 2^-14 of the largest magnitude of
 * their row (activations) or of their relation's [2d, d] matrix (weights); an element further down loses one bit per
 * factor of two and vanishes below 2^-38 of the largest.  Bound on a product sum_k x_k w_k: 3 * 2^-22 * sum |x_k w_k|
 * (the order of the fp32 fma chain it replaces) + 2^-38 * max|x| * sum_k |w_k| over the far-down x_k (and the same with x
 * and w exchanged).  The second term is invisible unless the large entries meet (near-)zero partners, e.g. one feature
 * 2^30 above the rest whose weight column is 0 — the reference's fp32 bmm (hypergnn.py:202,228) has no such case.
 * Three conditions are watched by every kernel that cuts rows or weights; each ORs a bit into the int32 device word
 * registered here (NULL: no guard):
 *   GHF_RANGE_ROWS / GHF_RANGE_WEIGHTS — per row / per relation matrix (per 32 x 32 tile in ghf_weights_pack_rs) the nonzero
 *     entries more than 2^14 below the largest are at least 1/8 of the nonzero entries;
 *   GHF_RANGE_WEAK_W — some relation's [W_msg; W_self] has an input row whose L1 norm is below d * 2^-16 of the largest
 *     row's (a half that is zero throughout, as in the backward's GHF_FLAG_ZERO_* passes, takes no part).
 * GUARANTEE while GHF_RANGE_WEAK_W is clear (s[k] = L1 norm of input row k, all s[k] >= d 2^-16 max s): summed over a
 * result row's d outputs, the second term is at most 2^-38 * max|x| * d * max s on either side, and sum_o sum_k |x_k w_ko| =
 * sum_k |x_k| s[k] >= max|x| * d 2^-16 * max s — i.e. the whole error stays within 4 * 2^-22 * sum |x_k w_ko|, the kind
 * of bound the fp32 fma chain has, however few or many entries of a row or a matrix lie far down.  A matrix with a weak
 * row is where a far-down entry can carry a result on its own (rows whose large entries meet that row); generated dense
 * weights do not have one.
 * The word belongs to the caller, who clears it before a forward and reads it after (the host mirror then repeats the
 * forward on the exact fp32 kernels when any bit is set).  One word per process (one process drives one GPU). */
#define GHF_RANGE_ROWS 1
#define GHF_RANGE_WEIGHTS 2
#define GHF_RANGE_WEAK_W 4
int ghf_set_range_flag(int32_t* device_word);

/* ---- K3 alone -------------------------------------------------------------------------
 * Replaces models/hypergnn.py:288-296 on rows [row0,row0+rows): agg already holds
 * out_v (GHF_FLAG_NO_TAIL output, e.g. after a cross-GPU reduction).  drop (training with dropout > 0, :293-294): the
 * mask, scaled by 1/(1-p), multiplied in between ReLU and LayerNorm; ghf_tail_bwd takes the same mask. */
int ghf_tail_fwd(const float* agg /* [N,d] */, const float* h /* [N,d] */,
                 const float* ln_gamma, const float* ln_beta, float ln_eps,
                 int64_t row0, int64_t rows, int d, float* h_out, const float* drop /* [N,d] or NULL */, void* stream);

/* ---- wide hidden sizes: the relation-stationary message layer (csrc/message_rs.hip) ---------------------------------
 * For d % 128 == 0, 128 <= d <= 1024 (ghf_message_rs_supported; BASELINE config 5, and d = 128 with many relations).  Same statement as
 * ghf_message_layer_fwd, in two passes over a CSR plan (block_nodes == 1):
 *   ghf_edge_transform_fwd: Y[ypos[k]] = h[src[k]] W_msg[r] + bias[r] + h[dst[k]] W_self[r] for the edges k in RELATION order
 *       (src / dst / ypos [E] int64: the edge's ends and its position in destination order); slice_tab [nslices][3] int64 =
 *       (relation, first edge, end edge) cuts every relation's range into tiles of at most 128 edges; WmT / WsT [R][d][d]
 *       are the weights TRANSPOSED ([r][out][in], ghf_transpose_batched of the natural layout); Y [E][d] fp32 scratch.
 *   ghf_edge_transform_h_fwd: the same per-edge results with the two-fp16-piece contraction of the d = 128 kernel (three
 *       16x16x32 products, 22 significand bits, 5x less matrix time): h_split = ghf_split_rows(h, GHF_WLAYOUT_SPLIT2H), w2h =
 *       ghf_weights_pack_rs(W_msg, W_self natural [R][d][d]) (ghf_weights_rs_bytes(R, d) bytes; shift_ws: R ints of scratch).
 *       Rows that stand for several edges (graphs with hubs): the layer is linear in the source rows, so the n edges of one
 *       (destination, relation) run need one row of this pass:  sum_e (h_u W_msg[r] + b[r] + h_v W_self[r]) =
 *       x W_msg[r] + n (b[r] + h_v W_self[r]),  x = the sum of the run's source rows.  ghf_run_rows_fwd writes those sums:
 *       x_split row i = sum of h[run_src[run_start[i] .. run_start[i+1])] (fp32, in that order) in ghf_split_rows form
 *       (ghf_split_rows_bytes(nruns, d, SPLIT2H) bytes).  A row k of this pass then has src[k] < 0 = row ~src[k] of x_split
 *       (NX rows; NULL / 0: none) and row_cnt[k] = n (float; NULL: every row is one edge).
 *   ghf_segment_partial_fwd (hubs only): P[slot] = sum(Y[first .. end)) for every (first, end, slot) of hub_chunks
 *       [nchunks][3] int64 — a destination with more rows than one wave should walk is summed in chunks first.
 *   ghf_segment_tail_fwd: rows [row0, row0+rows): out_v = sum(Y[off[v] .. off[v+1])) / max(indeg, 1), then the tail of
 *       ghf_tail_fwd (flags: GHF_FLAG_NO_TAIL / GHF_FLAG_RAW_SUM as for the message layer); off [N+1] int64.  Hubs:
 *       hub_of [N] int32 (hub index or -1; NULL = no hubs), hub_tab [H][2] int64 (first slot, slots) select rows of P
 *       to add instead of rows of Y; the mean divides by deg_of[v] (int32 [N]: the in-degree, when rows stand for several
 *       edges) or, deg_of == NULL, by off[v+1] - off[v].  h_split_out (optional): the rows
 *       written, also in ghf_split_rows(.., GHF_WLAYOUT_SPLIT2H) form for the next layer's ghf_edge_transform_h_fwd — a buffer
 *       of n_split rows (ghf_split_rows_bytes(n_split, d, GHF_WLAYOUT_SPLIT2H)). */
size_t ghf_weights_rs_bytes(int R, int d);
int ghf_weights_pack_rs(const float* W_msg, const float* W_self, int R, int d, void* w2h, int* shift_ws, void* stream);
int ghf_edge_transform_h_fwd(const void* h_split, int64_t N, int d, const int64_t* src, const int64_t* dst, const int64_t* ypos,
                             const int64_t* slice_tab, int64_t nslices, const void* w2h, int R, const float* bias,
                             const void* x_split, int64_t NX, const float* row_cnt, float* Y, void* stream);
int ghf_run_rows_fwd(const float* h, int64_t N, int d, const int64_t* run_src, const int64_t* run_start, int64_t nruns,
                     void* x_split, void* stream);
int ghf_segment_partial_fwd(const float* Y, const int64_t* hub_chunks, int64_t nchunks, int d, float* P, void* stream);
int ghf_message_rs_supported(int d);
int ghf_edge_transform_fwd(const float* h, int64_t N, int d, const int64_t* src, const int64_t* dst, const int64_t* ypos,
                           const int64_t* slice_tab, int64_t nslices, const float* WmT, const float* WsT, const float* bias,
                           float* Y, void* stream);
int ghf_segment_tail_fwd(const float* Y, const int64_t* off, const int32_t* deg_of, const int32_t* hub_of, const int64_t* hub_tab, const float* P,
                         const float* h, const float* ln_gamma, const float* ln_beta, float ln_eps, int64_t row0,
                         int64_t rows, int d, float* h_out, void* h_split_out, int64_t n_split, int flags, void* stream);

/* ---- backward of the path (the reference trains through it with autograd: demo.py:79-101) ----------
 * With out_v = (1/c_v) sum_e(h_u Wm[r] + b[r] + h_v Ws[r]), x = relu(out + h), h' = LayerNorm(x), g' = dL/dh':
 *   ghf_tail_bwd   : dpre = dL/d(out+h) (also the residual's share of dL/dh), G_v = dpre_v / c_v, and the LayerNorm's
 *                    dgamma_dbeta [2][d] = (sum_v g'_v * xhat_v, sum_v g'_v), summed in a fixed order on the way;  agg is the
 *                    forward's GHF_FLAG_NO_TAIL output (or agg_out).  G_split (optional): also G in the form ghf_split_rows
 *                    (GHF_WLAYOUT_SPLIT2H) would cut from it, for the gradient passes that gather G.  workspace:
 *                    ghf_tail_bwd_workspace_floats(N, d) floats
 *   ghf_group_outer: C[g][i][o] (+)= sum_{e in gstart[g]..gend[g]} A[ia[e]][i] * B[ib[e]][o]; ia / ib NULL = e itself,
 *                    da == 0: A = 1 (C is [ngroups][1][db]).  dWm[r] = sum h_u^T G_v, dWs[r], db[r], and the Linear
 *                    layers' weight gradients.  Summation order fixed: reproducible.
 *   ghf_colsum     : out[o] (+)= sum_v X[v][o] * (mask ? mask[v][o] > 0 : 1); workspace: ghf_colsum_workspace_floats
 *   ghf_relu_mask  : out = X * (ref > 0);   ghf_transpose_batched: out[b][j][i] = in[b][i][j]
 *   ghf_weights_pack: [top[r] ; bottom[r]] ([d,d] natural each, optionally transposed, NULL = zeros) -> weight layout
 *                    (the gradient with respect to h is ghf_message_layer_fwd with GHF_FLAG_RAW_SUM on transposed
 *                    weights: sum_{e->v} G_v Ws[r]^T on the plan, sum_{e: src=u} G_v Wm[r]^T on the reversed plan). */
/* Edge ids grouped (stably) by relation: perm [E], goff [R+1] (goff[r] = first position of relation r). */
size_t ghf_group_workspace_bytes(int64_t E);
int ghf_group_edges(const int64_t* rel_id, int64_t E, int R, void* workspace, size_t workspace_bytes,
                    int64_t* perm, int64_t* goff, void* stream);
size_t ghf_tail_bwd_workspace_floats(int64_t N, int d);
int ghf_tail_bwd(const float* grad_out, const float* agg, const float* h, const float* ln_gamma, float ln_eps,
                 const int32_t* indeg, int64_t N, int d, float* dpre, float* G, void* G_split /* or NULL */,
                 float* dgamma_dbeta /* [2][d] */, float* workspace, const float* drop /* [N,d] or NULL */, void* stream);
size_t ghf_colsum_workspace_floats(int64_t N, int d);
int ghf_colsum(const float* X, const float* mask, int64_t N, int d, float* workspace, float* out, int accumulate, void* stream);
int ghf_relu_mask(const float* X, const float* ref, int64_t n, float* out, void* stream);
int ghf_group_outer(const float* A, const int64_t* ia, int da, const float* B, const int64_t* ib, int db,
                    const int64_t* gstart, const int64_t* gend, int ngroups, float* C, int accumulate, void* stream);
/* The three per-relation gradients of a layer in one pass over the edges (d = 64 or a multiple of 128, tile by tile;
 * ghf_edge_outer_supported):
 *   dW[r] = sum_{e in r} [h[src[e]] | h[dst[e]]]^T G[dst[e]]   ([R][2d][d]: dW_msg[r] stacked on dW_self[r]),
 *   db[r] = sum_{e in r} G[dst[e]]                             ([R][d])
 * src / dst [E]: the edges grouped by relation (ghf_group_edges); slice_tab [nslices][3] = (relation, first edge, end edge)
 * cuts every relation's range into slices, relations ascending, never across a relation; slice_off [R+1] = first slice of
 * each relation.  workspace: nslices * (2*D*D + D) + 64 floats, D = min(d, 128).  Fixed summation order.  d = 64: exact fp32
 * (v_mfma_f32_16x16x4_f32); d % 128 == 0: two fp16 pieces per operand with ONE power-of-two scale per tensor (the largest
 * magnitude of h resp. G — found by the call — lifted into [2^13, 2^14)), three v_mfma_f32_16x16x32_f16 per product, fp32
 * accumulation: 22 significand bits relative to each tensor's largest entries.  N <= 0 keeps the exact fp32 chain at every d:
 * what the host mirror passes when a training step fell back to the exact kernels (range guard).
 * order (or NULL = table order): a permutation of 0 .. nslices-1, the slice each workgroup of the launch takes, in launch
 * order.  It changes no bit of the result (a slice's partial sums land at the slice's index, the reduction runs in table order)
 * — only which slices are resident together: with destinations ascending inside a relation, the slices ordered by their
 * position WITHIN their relation (then by relation) make the workgroups in flight read the same band of destination rows of
 * h and G, once from HBM and then out of the Infinity Cache, instead of every relation sweeping all rows on its own. */
int ghf_edge_outer_supported(int d);
int ghf_edge_outer(const float* h, const float* G, const int64_t* src, const int64_t* dst, const int64_t* slice_tab,
                   const int64_t* slice_off, const int32_t* order /* [nslices] or NULL */, int64_t nslices, int R, int d,
                   int64_t N /* rows of h and G */, float* workspace, float* dW, float* db, void* stream);
/* The same for a caller that holds the split forms of h and G (ghf_split_rows / the h_split_out of a layer / ghf_tail_bwd's
 * G_split): h_rowscale, G_rowscale [N] = their row scales (the N floats behind the N split rows).  The one scale per tensor is
 * then read off those (2^13 max_row 2^-s(row) has the exponent of the tensor's largest magnitude) instead of by a pass over
 * both tensors: same pieces, same products, same bits as ghf_edge_outer with N > 0.  N > 0 required.
 * Range guard (round 4): the row scales also say how many NONZERO rows of a tensor lie 2^-15 or more below its largest
 * magnitude — rows the one scale leaves below 0.5, where two fp16 pieces keep fewer than 22 bits.  Some such rows are normal
 * (a training step's G: the nodes the loss does not touch) and add 2^-15 of what the others add; when they are at least 7/8
 * of either tensor's nonzero rows — a few outlier rows set the scale and the bulk of the tensor would be cut short — the call
 * runs on the exact fp32 chain instead (the bits of N <= 0), decided on the device: both kernels are enqueued and the
 * workgroups of one return at once.  The four counters (far-down rows, nonzero
 * rows; of h, of G) stay in the workspace behind the partial sums and the two maxima:
 * ints at float offset nslices * (2*D*D + D) + 2. */
int ghf_edge_outer_scaled(const float* h, const float* G, const float* h_rowscale, const float* G_rowscale, const int64_t* src,
                          const int64_t* dst, const int64_t* slice_tab, const int64_t* slice_off, const int32_t* order,
                          int64_t nslices, int R, int d, int64_t N, float* workspace, float* dW, float* db, void* stream);
/* Elementwise pieces of the backward: out = X * exp(log_scale[0]) (log_scale on the device: the generator's learnable
 * scale, reference weight_generator.py:137-141); out = a + b (+ c when non-NULL); out[i][:] = g[i] * X[i][:] (the two
 * gradients of score_triple, reference hypergnn.py:304-318).  out may alias an input. */
int ghf_scale_exp(const float* X, int64_t n, const float* log_scale, float* out, void* stream);
int ghf_add3(const float* a, const float* b, const float* c, int64_t n, float* out, void* stream);
int ghf_rowscale(const float* X, const float* g, int64_t n, int d, float* out, void* stream);
/* out[v][:] = sum_{e = off[v] .. off[v+1]-1} w[iw[e]] * X[ix[e]][:]  (out [nseg,d], X [nx,d], off [nseg+1]; e ascending: fixed
 * order; ix clamped into [0, nx)).  The gradient of the fused edge scores (ghf_score_pairs_fwd with index arrays): per node, the
 * pairs it takes part in (grouped by ghf_group_edges with the node ids as keys). */
int ghf_segment_axpy(const float* w, const int64_t* iw, const float* X, const int64_t* ix, const int64_t* off, int64_t nseg,
                     int64_t nx, int d, float* out, void* stream);
/* out[0] = sum_i X[i] Y[i] (fixed order); workspace: (n + 8191) / 8192 floats */
int ghf_dot(const float* X, const float* Y, int64_t n, float* workspace, float* out, void* stream);
/* Hidden activations of the weight generator's three heads (what its backward needs besides the outputs):
 * acts[head][layer][r][Hh], layer = 0 .. num_hidden-1 (post-ReLU).  Same head_params as ghf_weightgen_fwd. */
int ghf_weightgen_acts(const float* text_emb, const float* const* head_params, int R, int T, int Hh, int num_hidden,
                       float* acts, const float* hidden_drop /* or NULL */, void* stream);
/* Backward of ghf_weightgen_fwd with GHF_WLAYOUT_NATURAL outputs (reference models/weight_generator.py:96-143 under plain
 * autograd), all three heads and all their layers in three launches.  outs[k] / grads[k] (k = message matrices, self matrices,
 * biases): the forward's outputs [R, d_in*d_out] (k < 2) / [R, d_out] and dL/d of them; log_scales[k]: the heads' log-scales
 * (device, 1 float each); acts: ghf_weightgen_acts' result; log_keep: NULL, or log(1/(1-p)) (device) when acts are post-dropout.
 * Writes dparams (one buffer per entry of head_params: dL/dW [out, in] and dL/db [out] of every layer), dls[k] (1 float each,
 * device: dL/d log-scale) and d_text_emb [R, T] (or NULL).  Exact fp32, fixed summation order.  text_dim and hidden_dim up to
 * 256 (ghf_weightgen_bwd_supported; wider generators: the per-operation chain — ghf_dot, ghf_scale_exp, ghf_relu_mask,
 * ghf_group_outer, ghf_colsum).  workspace: ghf_weightgen_bwd_workspace_floats floats. */
int ghf_weightgen_bwd_supported(int T, int Hh, int num_hidden);
size_t ghf_weightgen_bwd_workspace_floats(int R, int T, int Hh, int num_hidden, int d_in, int d_out);
int ghf_weightgen_bwd(const float* text_emb, const float* const* head_params, const float* acts, const float* const* outs,
                      const float* const* grads, const float* const* log_scales, int R, int T, int Hh, int num_hidden, int d_in,
                      int d_out, const float* log_keep, float* const* dparams, float* const* dls, float* d_text_emb,
                      float* workspace, void* stream);
/* Backward of ghf_text_encode_fwd: given te = its output and dte = dL/dte, writes dL/dchar_emb [V,C], dL/dW [T,C],
 * dL/db [T] (overwritten, fixed summation order).  workspace: 2*U*C + U*T floats. */
int ghf_text_encode_bwd(const int32_t* ids, const int32_t* lens, int U, int Lmax, const float* char_emb, int V, int C,
                        const float* W, int T, const float* te, const float* dte, float* workspace,
                        float* d_char_emb, float* dW, float* db, void* stream);
int ghf_transpose_batched(const float* in, int batch, int rows, int cols, float* out, void* stream);
int ghf_weights_pack(const float* top, const float* bottom, int transpose, int R, int d, int wlayout, float* out, void* stream);

/* ---- link-prediction scores ------------------------------------------------------------
 * Replaces models/hypergnn.py:304-318 (score_triple) and the row gathers of its call sites (demo.py:90-94,
 * score_triple(embs[src], embs[dst])):  scores[i] = sum_k a[ia[i]][k] * b[ib[i]][k],  i < n.
 * a [rows_a, d], b [rows_b, d] fp32 row-major (may be the same matrix); ia / ib int64 [n] or NULL (= i).
 * An index outside its matrix gives NaN for that pair (the reference raises from ATen). */
int ghf_score_pairs_fwd(const float* a, const float* b, const int64_t* ia, const int64_t* ib,
                        int64_t rows_a, int64_t rows_b, int64_t n, int d, float* scores, void* stream);

/* ---- link prediction against every node: rank counts and top-k (csrc/rank.hip) ----------------------
 * The step after training (demo.py:79-101 trains on pair scores): score query rows against ALL N candidate rows,
 *   s(i, j) = sum_k q[iq[i]][k] * c[j][k],  i < B, j < N   (fp32, accumulated in increasing k: the fmaf chain of
 *   v_mfma_f32_32x32x2_f32, the same bits as ghf_score_pairs_fwd's products summed in that order),
 * without ever storing the B x N scores.  q [rows_q, d], c [N, d] fp32 row-major (normally both the model's output);
 * iq int64 [B] or NULL (= i, then B <= rows_q); d <= 256 (GHF_EUNSUPPORTED beyond), B and N below 2^31.
 * Filter lists (the "filtered" setting: candidates known to be true, to be ignored) come in CSR form: filt_ptr int64
 * [B+1] ascending from 0, filt_idx int64 [nnz], nnz = filt_ptr[B] passed on the host side; each query's list sorted
 * ascending (an id may repeat: it is removed once).  nnz = 0 (both pointers may be NULL) means no lists.
 * An iq / target / filter id outside its range does not fault: that query's counts and ids are -1 (its top-k scores
 * NaN, as ghf_score_pairs_fwd).
 *
 * ghf_score_rank: with t_i = s(i, target[i]) and J_i = every row of c but target[i] and the rows in query i's list,
 *   greater[i] = #{j in J_i : s(i,j) > t_i},   equal[i] = #{j in J_i : s(i,j) == t_i}      (int64 [B]; NaN counts in neither).
 * Integer sums: bit-reproducible.  workspace: ghf_score_rank_workspace_bytes (0 = bad sizes), 256-byte aligned.
 *
 * ghf_score_topk: for 1 <= k <= 128 the k highest s(i, j) over j outside query i's list: scores [B, k] fp32 descending,
 * ids [B, k] int64, ties towards the lower id, (-inf, -1) where fewer than k candidates remain.  NaN and -inf scores are
 * never returned.  workspace: ghf_score_topk_workspace_bytes, 256-byte aligned (per query and candidate slab a list of
 * k + 256 entries). */
size_t ghf_score_rank_workspace_bytes(int64_t B, int64_t N, int d);
int ghf_score_rank(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                   const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, void* workspace,
                   size_t workspace_bytes, int64_t* greater, int64_t* equal, void* stream);
size_t ghf_score_topk_workspace_bytes(int64_t B, int64_t N, int d, int k);
int ghf_score_topk(const float* q, const float* c, const int64_t* iq, const int64_t* filt_ptr, const int64_t* filt_idx,
                   int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, int k, void* workspace, size_t workspace_bytes,
                   float* scores, int64_t* ids, void* stream);

/* ---- 1-vs-all softmax link-prediction loss against every node (csrc/softmax.hip) ---------------------
 * The differentiable counterpart of ghf_score_rank: the objective its filtered metrics measure.  q, c, iq, target and the
 * filter lists exactly as above, s(i, j) the same chain.  scale: a finite float > 0 (GHF_EINVAL otherwise).  With
 *   t_i = s(i, target[i]),   J_i = every row of c except the rows in query i's list — the target ALWAYS stays in J_i, even
 *   if it is listed; a repeated id in a list changes nothing —
 *   lse[i]  = log sum_{j in J_i} exp(scale s(i, j)),      loss[i] = lse[i] - scale t_i          (fp32 [B] each).
 * A listed candidate never enters the sum (it is not subtracted afterwards).  The B x N logits are never stored.
 * ghf_score_softmax_bwd: given grad_loss [B] and the forward's lse, with p_ij = exp(scale s(i,j) - lse[i]) for j in J_i
 * and 0 otherwise, and G_ij = grad_loss[i] scale (p_ij - [j = target[i]]):
 *   dq[i][:] = sum_j G_ij c[j][:]         [B, d], per query (NOT scattered through iq)
 *   dc[j][:] = sum_i G_ij q[iq[i]][:]     [N, d], every row written (zeros included: the caller does not clear it)
 * Limits as ghf_score_rank (d <= 256, GHF_EUNSUPPORTED beyond; B, N below 2^31).  An iq / target / filter id out of
 * range does not fault: that query's loss and lse are NaN and it contributes nothing to dq / dc (the backward takes a
 * NaN lse as "this query takes no part").  All sums run in a fixed order and there are no floating-point atomics: loss,
 * lse, dq and dc are bit-reproducible, and a query's loss and lse do not depend on the other queries of the call.
 * workspace: the matching _workspace_bytes query (0 = bad sizes), 256-byte aligned; O(B) plus 8 bytes per (query, candidate
 * slab) forward, one [B, d] partial of dq per candidate slab backward.  Nothing allocates or synchronises. */
size_t ghf_score_softmax_workspace_bytes(int64_t B, int64_t N, int d);
int ghf_score_softmax_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                          const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                          void* workspace, size_t workspace_bytes, float* loss, float* lse, void* stream);
size_t ghf_score_softmax_bwd_workspace_bytes(int64_t B, int64_t N, int d);
int ghf_score_softmax_bwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                          const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                          const float* lse, const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq, float* dc,
                          void* stream);

/* ---- multi-label 1-vs-all BCE link-prediction loss against every node (csrc/bce.hip, csrc/softmax.hip) --------
 * The 1-N objective of ConvE / TuckER / CompGCN: one query scored against every node, ALL of its known partners positives at
 * once, binary cross-entropy with label smoothing.  q, c, iq, rows_q, N, B, d and the limits exactly as ghf_score_softmax_fwd,
 * s(i, j) the same chain; there is no target.  The CSR lists have the shape of the filter lists (pos_ptr int64 [B+1] ascending
 * from 0, pos_idx int64 [nnz], every list sorted ascending) and name each query's positives P_i; an id that repeats counts
 * once; nnz = 0 (both pointers may be NULL) means no positives.  scale: a finite float > 0; smoothing: 0 <= smoothing < 1
 * (GHF_EINVAL otherwise).  With z_ij = scale s(i, j) and y_ij = (1 - smoothing) [j in P_i] + smoothing / N:
 *   loss[i] = sum_{j<N} softplus(z_ij) - (1 - smoothing) sum_{j in P_i} z_ij - (smoothing / N) sum_{j<N} z_ij      (fp32 [B])
 * = binary_cross_entropy_with_logits(z_i, y_i, reduction = "sum"); a mean over the candidates is the caller's division by N.
 * softplus(z) = max(z, 0) + log1p(exp(-|z|)) with a log1p that keeps its tail (far-negative logits still count).
 * ghf_score_bce_bwd: given grad_loss [B] and the forward's loss, with G_ij = grad_loss[i] scale (sigmoid(z_ij) - y_ij):
 *   dq[i][:] = sum_j G_ij c[j][:]         [B, d], per query (NOT scattered through iq)
 *   dc[j][:] = sum_i G_ij q[iq[i]][:]     [N, d], every row written (zeros included)
 * An iq or list id out of range does not fault (no id is dereferenced before it is range-checked): that query's loss is NaN
 * and it contributes nothing to dq / dc — the backward takes a NaN loss[i] as "this query takes no part" and reads nothing
 * else from loss.  All sums run in a fixed order, no floating-point atomics: loss, dq and dc are bit-reproducible, and a
 * query's loss does not depend on the other queries of the call.  workspace: the matching _workspace_bytes query (0 = bad
 * sizes), 256-byte aligned; O(B) plus 12 bytes per (query, candidate slab) forward, the softmax backward's size backward.
 * Nothing allocates or synchronises. */
size_t ghf_score_bce_workspace_bytes(int64_t B, int64_t N, int d);
int ghf_score_bce_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx, int64_t nnz,
                      int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, void* workspace,
                      size_t workspace_bytes, float* loss, void* stream);
size_t ghf_score_bce_bwd_workspace_bytes(int64_t B, int64_t N, int d);
int ghf_score_bce_bwd(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx, int64_t nnz,
                      int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, const float* loss,
                      const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq, float* dc, void* stream);

/* ---- the same four operations against a candidate subset (csrc/candidates.hip) --------------------------
 * Sampled or in-batch negatives for the two losses, type-constrained ranking for the two evaluations.  Every call above has
 * a _sub form that takes, beside the same arguments, the candidates as node ids:
 *   ic int64 [C], STRICTLY ascending, every id in [0, N);  1 <= C <= N (GHF_EINVAL otherwise).
 * With P the set of ids in ic, the result is that of the call above on the table c[ic] — except that every id that goes in
 * (target, the lists) or comes out (top-k ids) stays a row id of c, and list entries outside P take no part:
 *   ghf_score_rank_sub         counts j in P outside query i's list and other than target[i].  The target may be ANY row of
 *                              c, a candidate or not: t_i comes from its own row.
 *   ghf_score_topk_sub         the k best of P outside the list, ties towards the lower id, (-inf, -1) where fewer remain.
 *   ghf_score_softmax_fwd_sub  J_i = (P minus query i's list) plus target[i], and the target must be in P: a query whose
 *                              target is not (or is out of range) has loss = lse = NaN and takes no part in the backward.
 *   ghf_score_bce_fwd_sub      the loss over P alone: positives are the listed ids inside P, y_ij = (1 - smoothing) [listed]
 *                              + smoothing / C, sums over j in P; a mean over the candidates is the caller's division by C.
 *   the two backwards          dq [B, d] as above; dc is [C, d], row j the gradient of row ic[j] of c, every row written.
 * No [C, d] copy of the candidate rows is made: the sweeps read candidate j at c + ic[j] d.  Geometry (slabs, partial sums)
 * is that of the calls above for N := C, so the bits of a subset call equal those of the call above on a contiguous copy
 * c[ic] with renumbered ids, a query's bits do not depend on its batch, and everything stays bit-reproducible (no
 * floating-point atomics).  A list id outside [0, N) makes its query invalid, as above.  An ic that is not strictly
 * ascending or leaves [0, N) makes EVERY query invalid (counts and ids -1, scores / losses NaN, dq and dc zero); no row
 * outside c is read or written whatever ic holds.  workspace: the matching _sub_workspace_bytes query, which also takes nnz
 * (the renumbered lists live there); 0 = bad sizes; 256-byte aligned.  Nothing allocates or synchronises. */
size_t ghf_score_rank_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz);
int ghf_score_rank_sub(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                       const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, const int64_t* ic,
                       int64_t C, void* workspace, size_t workspace_bytes, int64_t* greater, int64_t* equal, void* stream);
size_t ghf_score_topk_sub_workspace_bytes(int64_t B, int64_t C, int d, int k, int64_t nnz);
int ghf_score_topk_sub(const float* q, const float* c, const int64_t* iq, const int64_t* filt_ptr, const int64_t* filt_idx,
                       int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, int k, const int64_t* ic, int64_t C,
                       void* workspace, size_t workspace_bytes, float* scores, int64_t* ids, void* stream);
size_t ghf_score_softmax_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz);
int ghf_score_softmax_fwd_sub(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                              const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                              const int64_t* ic, int64_t C, void* workspace, size_t workspace_bytes, float* loss, float* lse,
                              void* stream);
size_t ghf_score_softmax_bwd_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz);
int ghf_score_softmax_bwd_sub(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                              const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                              const float* lse, const float* grad_loss, const int64_t* ic, int64_t C, void* workspace,
                              size_t workspace_bytes, float* dq, float* dc, void* stream);
size_t ghf_score_bce_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz);
int ghf_score_bce_fwd_sub(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx,
                          int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, const int64_t* ic,
                          int64_t C, void* workspace, size_t workspace_bytes, float* loss, void* stream);
size_t ghf_score_bce_bwd_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz);
int ghf_score_bce_bwd_sub(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx,
                          int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, const float* loss,
                          const float* grad_loss, const int64_t* ic, int64_t C, void* workspace, size_t workspace_bytes, float* dq,
                          float* dc, void* stream);

/* ---- the same four operations with a per-candidate bias (csrc/rank_sweep.h) -----------------------------
 * A log-Q correction for sampled negatives, a learned entity bias (the b_t of ConvE / TuckER / CompGCN's f(h, r) . e_t + b_t),
 * a prior or soft mask at evaluation.  Every call above has a _b form that takes the arguments of its _sub form plus
 *   bias fp32 [N], one entry per ROW of c (a node id, also when ic is given);  NULL is GHF_EINVAL.
 *   ic = NULL with C = 0 means every node (the result of the plain call with the bias); otherwise ic as for the _sub calls.
 * With s(i, j) the chain above, unchanged:
 *   ghf_score_rank_b, ghf_score_topk_b   s_b(i, j) = fl32(s(i, j) + bias[j]): ONE fp32 add behind the chain.  t_i is formed the
 *                              same way from the target's own row and its own bias entry, a candidate or not.  Top-k returns
 *                              the biased scores.  Ties, (-inf, -1) padding and the lists as above.
 *   ghf_score_softmax_fwd_b, ghf_score_bce_fwd_b   z_ij = fmaf(scale, s(i, j), bias[j]) wherever the calls above use
 *                              scale s(i, j): the lse, loss = lse - z_it, BCE's three sums.  The bias is NOT multiplied by scale;
 *                              labels and smoothing / N as above.
 *   the two backwards          G_ij as above with the biased z (the softmax forms p_ij = exp(fmaf(scale, s, bias[j] - lse[i])));
 *                              dq and dc as above, and db [N] ([C] with ic, entry j belonging to node ic[j]; NULL = not wanted):
 *                              db[j] = sum_i grad_loss[i] (p_ij - [j = target[i]])      softmax
 *                              db[j] = sum_i grad_loss[i] (sigma(z_ij) - y_ij)          BCE
 *                              computed as (sum_i G_ij) / scale over the queries in ascending order by the dc pass: every entry
 *                              written, no floating-point atomics, bit-reproducible.
 * bias[j] = -inf on a candidate that is no query's target takes it out: rank counts it in neither count, top-k never returns
 * it, the softmax adds 0 for it and its dc row and db entry are exactly 0.  For the BCE loss the bias must be finite.  A NaN
 * entry is outside the contract but faults nothing.  No value is checked on the host.  A bias of zeros returns the bits of
 * the call without one (fmaf(scale, s, 0) = fl(scale s), s + 0 = s).  Errors as above: a bad id makes its query invalid, a bad
 * ic every query (db is then zero).  workspace: the matching _b_workspace_bytes query (B, N, C, ...; C = 0: every node), which
 * with C > 0 holds the _sub workspace and the bias gathered through ic, [C] floats; 0 = bad sizes; 256-byte aligned.  Nothing
 * allocates or synchronises. */
size_t ghf_score_rank_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz);
int ghf_score_rank_b(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                     const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, const int64_t* ic,
                     int64_t C, const float* bias, void* workspace, size_t workspace_bytes, int64_t* greater, int64_t* equal,
                     void* stream);
size_t ghf_score_topk_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int k, int64_t nnz);
int ghf_score_topk_b(const float* q, const float* c, const int64_t* iq, const int64_t* filt_ptr, const int64_t* filt_idx,
                     int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, int k, const int64_t* ic, int64_t C,
                     const float* bias, void* workspace, size_t workspace_bytes, float* scores, int64_t* ids, void* stream);
size_t ghf_score_softmax_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz);
int ghf_score_softmax_fwd_b(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                            const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                            const int64_t* ic, int64_t C, const float* bias, void* workspace, size_t workspace_bytes, float* loss,
                            float* lse, void* stream);
size_t ghf_score_softmax_bwd_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz);
int ghf_score_softmax_bwd_b(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                            const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                            const float* lse, const float* grad_loss, const int64_t* ic, int64_t C, const float* bias,
                            void* workspace, size_t workspace_bytes, float* dq, float* dc, float* db, void* stream);
size_t ghf_score_bce_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz);
int ghf_score_bce_fwd_b(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx,
                        int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, const int64_t* ic,
                        int64_t C, const float* bias, void* workspace, size_t workspace_bytes, float* loss, void* stream);
size_t ghf_score_bce_bwd_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz);
int ghf_score_bce_bwd_b(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx,
                        int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, const float* loss,
                        const float* grad_loss, const int64_t* ic, int64_t C, const float* bias, void* workspace,
                        size_t workspace_bytes, float* dq, float* dc, float* db, void* stream);

/* ---- negative-sampling loss with self-adversarial weighting (csrc/negsamp.hip, csrc/softmax.hip) -----------
 * The objective of RotatE, PyKEEN's NSSALoss, DGL-KE and the OGB wikikg2 / biokg baselines on one shared set of negatives;
 * adv_temperature = 0 is the uniform negative-sampling loss of TransE / word2vec.  One general form per call: q, c, iq,
 * target, the filter lists, rows_q, N, B, d and the limits exactly as ghf_score_softmax_fwd; ic [C] as for the _sub calls, or
 * ic = NULL with C = 0 for every node; bias [N] as for the _b calls, or NULL for none (GHF_EINVAL for any other pairing of ic
 * and C).  s(i, j) is the same chain, z_ij = scale s(i, j), or fmaf(scale, s(i, j), bias[j]) with a bias (NOT multiplied by
 * scale).  scale: finite, > 0; margin: finite; adv_temperature (alpha): finite, >= 0; GHF_EINVAL otherwise.  The bias must be
 * finite, as for the BCE loss.  With P the candidates (every row of c, or ic) and J_i = P minus query i's list minus
 * target[i] — known partners are filtered out, the target is never its own negative:
 *   lw[i]   = log sum_{j in J_i} exp(alpha z_ij)                                  fp32 [B]; -inf when J_i is empty
 *   w_ij    = exp(alpha z_ij - lw[i])                                             sums to 1 over J_i; alpha = 0: 1 / |J_i|
 *   loss[i] = softplus(-(z_it + margin)) + sum_{j in J_i} w_ij softplus(z_ij + margin)                       fp32 [B]
 * "positive term + weighted negative term": PyKEEN's / 2 and the mean over the batch are the caller's.  A query without
 * negatives has the positive term alone.  softplus as for the BCE loss.
 * ghf_score_negsamp_bwd: given grad_loss [B] and the forward's lw, THE WEIGHTS ARE CONSTANTS (detached, as in RotatE and
 * PyKEEN; part of the contract):
 *   G_ij = grad_loss[i] scale w_ij sigmoid(z_ij + margin)  on J_i,   G_it = -grad_loss[i] scale sigmoid(-(z_it + margin)),
 *   G_ij = 0 at a listed j;   dq[i] = sum_j G_ij c[j]  [B, d] (NOT scattered through iq),   dc[j] = sum_i G_ij q[iq[i]]
 *   ([N, d], or [C, d] with ic, row j the gradient of row ic[j] of c; every row written),   db[j] = (sum_i G_ij) / scale  ([N] or
 *   [C]; NULL = not wanted; ignored without a bias).
 * With ic the target must be in P: a query whose target is not, or whose iq / target / list id is out of range, has loss = lw
 * = NaN and takes no part in the backward, which reads a NaN lw[i] as "no part" and an lw[i] of -inf as "the target entry
 * alone".  An ic that is not strictly ascending or leaves [0, N) makes every query invalid.  No id faults.  All sums run in a
 * fixed order, no floating-point atomics: loss, lw, dq, dc and db are bit-reproducible; the slabs depend on the candidate
 * count and d alone, so a query's bits do not depend on its batch, and a subset call has the bits of the all-node call on a
 * contiguous copy c[ic].  A bias of zeros gives the bits of the call without one.  workspace: the matching _workspace_bytes
 * query (C = 0: every node; 0 = bad sizes, d > 256 included), 256-byte aligned: O(B) plus 12 bytes per (query, candidate
 * slab) forward, the softmax backward's backward, plus the id map and C floats with C > 0.  d > 256 is GHF_EUNSUPPORTED.
 * Nothing allocates or synchronises. */
size_t ghf_score_negsamp_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz);
int ghf_score_negsamp_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                          const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                          float margin, float adv_temperature, const int64_t* ic, int64_t C, const float* bias, void* workspace,
                          size_t workspace_bytes, float* loss, float* lw, void* stream);
size_t ghf_score_negsamp_bwd_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz);
int ghf_score_negsamp_bwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                          const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                          float margin, float adv_temperature, const float* lw, const float* grad_loss, const int64_t* ic,
                          int64_t C, const float* bias, void* workspace, size_t workspace_bytes, float* dq, float* dc, float* db,
                          void* stream);

/* ---- relation-typed query rows (csrc/relation.hip) ----------------------------------------------------
 * No counterpart in the reference, whose score_triple (models/hypergnn.py:304-318) ignores the relation.  The query side of
 * a (head, relation, ?) score: every query row multiplied by ITS relation's matrix, without gathering a matrix per query
 * (the [B, d, d] operand of torch.bmm(x[ix].unsqueeze(1), W[rel])):
 *   out[i][:] = [GHF_REL_ADD_X] x[ix[i]][:]  +  x[ix[i]][:] @ op(W[rel[i]])  +  [bias != NULL] bias[rel[i]][:],     i < B
 * x [rows_x, d] fp32 row-major; ix int64 [B] or NULL (= i, then B <= rows_x); rel int64 [B]; W [R, d, d] natural
 * (W[r][k][l]: input k, output l); op = identity, or the transpose with GHF_REL_TRANSPOSE (out[l] = sum_k x[k] W[r][l][k]:
 * the gradient with respect to the rows, dx = g + g @ W[r]^T, is this same call); bias [R, d] or NULL; out [B, d].
 * 1 <= d <= 256 (the range of the rank calls; GHF_EUNSUPPORTED beyond), 0 < B < 2^31, 0 < R < 2^23.
 * perm [B] / goff [R + 1]: the queries grouped by relation, exactly what ghf_group_edges gives for (rel, B, R).  They are
 * PASSED IN, not computed here: the caller's backward needs the same grouping (ghf_group_outer over the relation groups),
 * so one sort serves the forward and both gradient calls.  A row that perm does not list is not written.
 * workspace: ghf_relation_rows_workspace_bytes(B, R) bytes (0 = bad sizes), 256-byte aligned: the table of (relation, tile
 * of <= 64 grouped rows) work items, cut from goff on the device; the launch is sized by its bound ceil(B/64) + R on the
 * host.  Nothing allocates, reads back or synchronises: the call is capturable.
 * An ix[i] or rel[i] out of range does not fault: that row of out is NaN and no other row is touched by it (goff and perm
 * are clamped as well: a malformed grouping cannot make the kernels read or write out of bounds).
 * Numerics: out[i][l] = (x[l] + s) + bias[l] with s the fp32 chain s = fmaf(x[k], op(W)[k][l], s), k = 0 .. d-1, from 0 —
 * v_mfma_f32_16x16x4_f32, the tail of k padded with zeros.  A row of out depends on its own x row, W[r] and bias[r] only,
 * bit for bit: never on the other queries of the call or on its place among them.  No atomics. */
#define GHF_REL_ADD_X     1   /* add the row itself (the residual) */
#define GHF_REL_TRANSPOSE 2   /* multiply by W[r]^T */
size_t ghf_relation_rows_workspace_bytes(int64_t B, int R);
int ghf_relation_rows(const float* x, const int64_t* ix /* [B] or NULL */, const int64_t* rel /* [B] */, const float* W /* [R,d,d] */,
                      const float* bias /* [R,d] or NULL */, const int64_t* perm /* [B] */, const int64_t* goff /* [R+1] */,
                      int64_t rows_x, int64_t B, int R, int d, int flags, void* workspace, size_t workspace_bytes,
                      float* out /* [B,d] */, void* stream);

/* ---- relation prediction: every relation's score for a pair (csrc/relation_predict.hip) -----------------
 * Which relation holds between two given nodes, (head, ?, tail).  With a = x[ia[i]], b = x[ib[i]]:
 *   out[i][u] = sum_l q_l b_l,   q = [GHF_REL_ADD_X] a  +  a @ op(W[u])  +  [bias != NULL] bias[u],     i < B, u < U
 * x [rows_x, d]; ia, ib int64 [B]; W [U, d, d] natural; op = identity or the transpose (GHF_REL_TRANSPOSE); bias [U, d] or
 * NULL; out [B, U] fp32, addressed with 64 bits.  1 <= d <= 256 (GHF_EUNSUPPORTED beyond), 0 < B < 2^31, 0 < U < 2^23.
 * One sweep: every (64-row query tile, relation) multiplies on v_mfma_f32_16x16x4_f32 and ends in a dot product in the
 * epilogue; only the [B, U] table is written.  The [B, U, d] operand of einsum("bi,uij->buj", x[ia], W) does not exist.
 * Numerics: q_l is bit for bit the element ghf_relation_rows gives for (ix = ia[i], rel = u, the same flags): the chain
 * s = fmaf(a[k], op(W[u])[k][l], s), k = 0 .. d-1 from 0, then (a_l + s) + bias[u][l].  The sum over l has one fixed order:
 * with DC = d rounded up to 64, p_c = the chain fmaf(q_l, b_l, p_c) over l = c, c + 16, .. < DC ascending from 0 (q = b = 0
 * past d), c < 16; then t_c = p_c + p_(c^1); v_c = t_c + t_(c^2); w_c = v_c + v_(7-c) (c < 8; likewise in 8..15);
 * out = w_0 + w_15.  An entry depends on its own two rows, W[u] and bias[u] only, bit for bit: not on the batch, the tile or
 * the other relations of the call.  An ia[i] or ib[i] out of range does not fault (ids are tested before any address is
 * formed): that row of out is NaN and no other row is touched.  Nothing allocates, reads back or synchronises.
 *
 * Backward, given G [B, U] (= d loss / d out).  Fixed summation orders, no floating-point atomics: bit-reproducible.
 *   ghf_relation_scores_bwd_rows:     out[i][:] = sum_u G[i][u] q(i, u)[:], u ascending, [B, d] — the sweep with "add G q to
 *     the row" as its epilogue.  As called it is d loss / d b rows; with ia := ib, the flags' transpose flipped and bias = NULL
 *     it is d loss / d a rows = sum_u G[i][u] (b + b @ op(W[u])^T).  When the tiles alone would leave the machine idle the
 *     relations of a tile are split over workgroups and the partials ([splits, B, d], in the workspace; the split count is
 *     bounded so that they never reach B x U x d) are added in split order.  A bad ia[i]: NaN row.
 *   ghf_relation_scores_bwd_weights:  dW[u] = sum_i G[i][u] a_i^T b_i  [U, d, d],  dbias[u] = sum_i G[i][u] b_i  [U, d] (or
 *     NULL), i ascending: a GEMM whose contraction runs over the queries, the G-scaled a rows against the b rows.  Slabs of
 *     queries (partials in the workspace, added in slab order).  A query with an id out of range adds nothing.  flags: none
 *     defined, must be 0.  (For op = transpose pass ia and ib swapped and read dW as the gradient of W; dbias then needs
 *     its own call: the decoder never transposes.)
 * workspace: the matching _workspace_bytes query (works without a GPU; 0 = bad sizes), 256-byte aligned. */
int ghf_relation_scores(const float* x, const int64_t* ia /* [B] */, const int64_t* ib /* [B] */, const float* W /* [U,d,d] */,
                        const float* bias /* [U,d] or NULL */, int64_t rows_x, int64_t B, int64_t U, int d, int flags,
                        float* out /* [B,U] */, void* stream);
size_t ghf_relation_scores_bwd_rows_workspace_bytes(int64_t B, int64_t U, int d);
int ghf_relation_scores_bwd_rows(const float* x, const int64_t* ia, const float* G /* [B,U] */, const float* W, const float* bias,
                                 int64_t rows_x, int64_t B, int64_t U, int d, int flags, void* workspace, size_t workspace_bytes,
                                 float* out /* [B,d] */, void* stream);
size_t ghf_relation_scores_bwd_weights_workspace_bytes(int64_t B, int64_t U, int d);
int ghf_relation_scores_bwd_weights(const float* x, const int64_t* ia, const int64_t* ib, const float* G /* [B,U] */, int64_t rows_x,
                                    int64_t B, int64_t U, int d, int flags, void* workspace, size_t workspace_bytes,
                                    float* dW /* [U,d,d] */, float* dbias /* [U,d] or NULL */, void* stream);

/* ---- the sparse row exchange of the multi-GPU forward (no counterpart in the single-process reference) ----
 * packed[i] = rows[idx[i]] (row_bytes, a multiple of 16) followed by extra[idx[i]] (extra_bytes, a multiple of 4; extra may be
 * NULL with extra_bytes = 0), i < n: the listed rows of a [nrows, row_bytes] table (and of a second table indexed alike — the
 * split form's scales) as one contiguous message; ghf_rows_unpack writes a received message to the rows' places.  idx: int64,
 * distinct for unpack (entries outside [0, nrows) are skipped).  Bit-exact copies.  n = 0 is an empty message: nothing is
 * read or written, idx and packed may be NULL. */
int ghf_rows_pack(const void* rows, int64_t row_bytes, const void* extra, int64_t extra_bytes, const int64_t* idx, int64_t n,
                  int64_t nrows, void* packed, void* stream);
int ghf_rows_unpack(const void* packed, const int64_t* idx, int64_t n, int64_t nrows, void* rows, int64_t row_bytes, void* extra,
                    int64_t extra_bytes, void* stream);
/* The adjoint of the exchange (training across GPUs): rows[idx[i]][k] += packed[i][k] (fp32), i < n, k < d; idx NULL = row i
 * itself.  idx entries distinct within one call (no atomics; callers add the peers' messages one call after another, in
 * rank order); entries outside [0, nrows) skipped.  d a multiple of 4, 16-byte aligned buffers.  One fp32 add per element. */
int ghf_rows_accumulate(const float* packed, const int64_t* idx, int64_t n, int64_t nrows, float* rows, int d, void* stream);
/* The same sum for rows of ANY width d > 0 and buffers aligned to 4 bytes: where d is a multiple of 4 and both buffers are
 * 16-byte aligned it is the call above, bit for bit; otherwise one float per lane.  The losses' candidate subsets put their
 * [C, d] gradient back into the table's rows with it: they take every d <= 256, not only whole float4s. */
int ghf_rows_accumulate_any(const float* packed, const int64_t* idx, int64_t n, int64_t nrows, float* rows, int d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GHF_H */
