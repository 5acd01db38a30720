/*
 * stellar_rw.h — C ABI of libstellar_rw.so, the MI355X-native (gfx950) engine behind the
 * `--cmd randomwalk` path of data61/stellar-random-walk.
 *
 * The reference has no FFI of its own (it is 100 % Scala on Spark); its seams for this path are the
 * Scala-level interfaces cited next to each entry point below.  A JNI shim
 * (Java_au_csiro_data61_randomwalk_algorithm_HipRandomWalk_*) binds exactly these functions — see
 * INTEGRATION.md.  Paths: M/ = randomwalk/src/main/scala/au/csiro/data61/randomwalk/.
 *
 * Conventions: plain C, no exceptions cross the boundary; every function returns an srw status
 * (0 = ok) and srw_last_error() gives the message.  The opaque handle owns all device memory; the
 * caller owns every buffer it passes in.  A handle is single-threaded; distinct handles may be used
 * from distinct threads.  There is NO CPU fallback: every compute entry point runs HIP kernels on the
 * handle's device and fails with SRW_ERR_HIP when no gfx950 device is usable.
 */
#ifndef STELLAR_RW_H
#define STELLAR_RW_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srw_handle srw_handle;

enum {
  SRW_OK = 0,
  SRW_ERR_INVALID = 1, /* bad argument / bad state */
  SRW_ERR_IO = 2,      /* file cannot be opened / written */
  SRW_ERR_PARSE = 3,   /* an input line on which the reference job throws (NumberFormatException ...) */
  SRW_ERR_HIP = 4,     /* HIP runtime error, or no usable GPU */
  SRW_ERR_EXISTS = 5,  /* <output>/path already exists (FileAlreadyExistsException in the reference) */
  SRW_ERR_NOMEM = 6
};

/* sampler selection */
enum {
  SRW_SAMPLER_REFERENCE = 0, /* Mode R: reference-exact linear-CDF inversion (bit-identical paths) */
  SRW_SAMPLER_ALIAS = 1      /* Mode A: per-vertex alias tables + rejection (statistically identical) */
};
/* RNG selection.  The reference's only determinism hook is the injected nextFloat closure
 * (M/algorithm/RandomSample.scala:5, M/algorithm/RandomWalk.scala:51-52,75-76). */
enum {
  SRW_RNG_CONST = 0,  /* nextFloat = () => const_r, as the reference's tests inject */
  SRW_RNG_PHILOX = 1  /* Philox4x32-10, key (seed,0), ctr (walk iteration, source id, step index, 0),
                         u = (x0 >> 8) * 2^-24 (same 24-bit lattice as java.util.Random.nextFloat) */
};

typedef struct {
  int32_t device; /* HIP device ordinal */
  int32_t rank;   /* vertex sharding: this handle stores the rows of the vertices v with owner(v) == rank,   */
  int32_t world;  /*   owner(v) = mix32(v) mod world — the role of HashPartitioner (RandomWalk.scala:16), with */
                  /*   the ids mixed first so that skewed id spaces (RMAT: hubs at round ids) stay balanced;  */
                  /*   world = 1 keeps the whole graph (single-GPU and replicated modes)                       */
  int32_t flags;  /* SRW_CFG_* */
} srw_config;
enum {
  /* sharded handles (world > 1): a vertex is owned by the partition id recorded for it by a partitioned load
   * (VCutRandomWalk: GraphMap.getPartition(steps.last), M/algorithm/VCutRandomWalk.scala:121-134), modulo world;
   * vertices without a recorded partition fall back to mix32(v) mod world. */
  SRW_CFG_OWNER_FROM_PARTITIONS = 1,
  /* whole-graph handles (world == 1): always compact the vertex ids at load (slot = rank among the sorted distinct ids).
   * Without the flag this happens only when the id space is sparse — the reference's HashMap-keyed GraphMap
   * (M/algorithm/GraphMap.scala:13-15) takes any int32 ids, e.g. "-2147483648 2147483647".  Results are the same
   * either way (the Philox stream stays keyed by the input's ids); the flag exists for tests. */
  SRW_CFG_COMPACT_IDS = 2,
  /* sharded handles (world > 1): do NOT build the replicated membership structure (the sorted neighbor ids of the WHOLE
   * graph on every shard: 4 B per adjacency entry + 16 B per id slot, and the largest sort of the load).  It is what a
   * shard needs to evaluate "x in N(prev)" for a prev it does not own, i.e. only when q != 1
   * (M/algorithm/RandomSample.scala:37); walks with q == 1 (config 4: p = q = 1) never read it.  A walk with q != 1 on
   * such a handle fails with SRW_ERR_INVALID.  With the flag a shard's memory is proportional to 1/world. */
  SRW_CFG_NO_MEMBERSHIP = 4,
  /* sharded handles (world > 1): owner(v) = nonNegativeMod(v, world) — org.apache.spark.HashPartitioner over as many partitions as
   * there are GPUs, the partition map of the reference (RandomWalk.scala:16, UniformRandomWalk.scala:42: partitionBy(new
   * HashPartitioner(rddPartitions)) on Int keys, whose hashCode is the value) — instead of the default mix32(v) mod world.
   * Results are the same under any owner function (tests); the default mixes the ids first because the low bits of an unpermuted
   * RMAT id correlate with the degree (one shard of eight gets 17 % of the walkers).  Ignored when the ids are compacted or a VCut
   * partition table is in force. */
  SRW_CFG_OWNER_HASH_PARTITIONER = 8
};

/* Replaces: SparkContext + GraphMap singleton lifetime (M/Main.scala:21-23, M/algorithm/GraphMap.scala:11). */
int32_t srw_create(const srw_config *cfg, srw_handle **out);
void srw_destroy(srw_handle *h);
/* Message of the last failure on h (h may be NULL for srw_create failures). */
const char *srw_last_error(const srw_handle *h);
/* Launch all kernels on this hipStream_t (default: the handle's own stream). */
int32_t srw_set_stream(srw_handle *h, void *hip_stream);

/* The job's --numWalks (M/common/Params.scala:7-23, default 10): how many walk iterations will run over the sampling
 * tables that the next srw_walk* call builds for its (p, q) — a caller that walks the job in several calls (one iteration
 * per call, batches) announces the total here.  It only steers what is worth BUILDING (the finer per-edge tables of the
 * biased walk cost ~8 s at config 3 and save ~0.1 s per iteration: they are built from 64 planned iterations on); results
 * never depend on it.  0 = unknown: the reference's default (10), or the call's own num_walks if that is larger. */
int32_t srw_plan_walks(srw_handle *h, int64_t num_walks);

/* ---- graph load ---------------------------------------------------------------------------- */
/* Replaces UniformRandomWalk.loadGraph (M/algorithm/UniformRandomWalk.scala:17-88) and, with
 * partitioned != 0, VCutRandomWalk.loadGraph (M/algorithm/VCutRandomWalk.scala:13-98): parses the
 * edge-list text with the reference's token rules, builds the adjacency in HBM as CSR with every
 * neighbor list in input-line order, multi-edges and self-loops kept.  Files of two integer columns (plus, with
 * weighted, a short decimal weight column) are tokenized on the GPU; every other shape and every malformed file
 * goes through the host tokenizer, with identical results and errors (SRW_HOST_TOKENIZER=1 forces the host). */
int32_t srw_load_edgelist(srw_handle *h, const char *path, int32_t directed, int32_t weighted,
                          int32_t partitioned, int32_t rdd_partitions);
/* Same construction from already-parsed lines in file order (host pointers).  w may be NULL (1.0f),
 * pid may be NULL.  Replaces the flatMap/reduceByKey stage, UniformRandomWalk.scala:26-41. */
int32_t srw_load_coo(srw_handle *h, const int32_t *src, const int32_t *dst, const float *w,
                     const int32_t *pid, int64_t n_lines, int32_t directed);
/* The same lines already in device memory on the handle's GPU (the edge_index of a training loop; no reference counterpart): builds
 * exactly the graph srw_load_coo builds from the same values with pid == NULL — rows, order, weight bits, srw_graph_stats, compacted
 * sparse ids, the owner-filtered build of a sharded handle.  d_src / d_dst: n_lines ids each, int32 or int64 by id_type, each pointer
 * aligned to its element only (the rows of a contiguous [2][n_lines] array are d_src and d_src + n_lines); d_w: n_lines floats or NULL
 * (1.0f).  The arrays are only read.  The work is ordered on the handle's stream — the caller has made sure that the arrays are
 * written before the call.  One kernel finds the id range and narrows int64 ids (csrc/coo_ingest.hip); int32 lines with dense ids on
 * a whole-graph handle are not copied at all.  SRW_ERR_INVALID, with the graph loaded before still loaded: a NULL d_src / d_dst with
 * n_lines > 0, n_lines < 0, an unknown id_type, a misaligned pointer, an int64 id outside int32 (the message names the first such
 * line index, its column and the id). */
enum { SRW_IDS_I32 = 0, SRW_IDS_I64 = 1 };
int32_t srw_load_coo_device(srw_handle *h, const void *d_src, const void *d_dst, const float *d_w,
                            int64_t n_lines, int32_t id_type, int32_t directed);
/* Complete adjacency rows, the GraphMap.addVertex surface (M/algorithm/GraphMap.scala:23-56,83-85):
 * row i is vertex vids[i] with neighbors [offs[i], offs[i+1]); first occurrence of a vertex wins. */
int32_t srw_load_adjacency(srw_handle *h, const int32_t *vids, const int64_t *offs, int64_t n_rows,
                           const int32_t *ids, const float *w, const int32_t *pids);
/* Synthetic RMAT (a,b,c,d)=(.57,.19,.19,.05) generated on the device straight into COO -> CSR
 * (BASELINE.md §4).  Edge i is a pure function of (seed, i), so any rank can generate any slice. */
int32_t srw_generate_rmat(srw_handle *h, int32_t scale, int64_t n_edges, uint32_t seed, int32_t weighted,
                          int32_t directed);

/* nVertices / nEdges as the reference prints them ("vertices: N", "edges: N",
 * UniformRandomWalk.scala:69-72); int64 because the reference's Int counters overflow at C4. */
int32_t srw_graph_stats(const srw_handle *h, int64_t *n_vertices, int64_t *n_entries);
/* Present vertex ids, ascending (the walker seeds, UniformRandomWalk.scala:81-87). out[n_vertices]. */
int32_t srw_graph_vertices(const srw_handle *h, int32_t *out);
/* GraphMap.getNeighbors (M/algorithm/GraphMap.scala:109-120): *n = -1 for `null` (unknown vertex),
 * 0 for a vertex without out-edges, else the list length; copies at most cap entries. */
int32_t srw_graph_neighbors(const srw_handle *h, int32_t v, int32_t *ids, float *w, int64_t cap, int64_t *n);
/* GraphMap.getPartition (:66-68): *pid = last partition id recorded for dst v, *known = 0 if none. */
int32_t srw_graph_partition(const srw_handle *h, int32_t v, int32_t *pid, int32_t *known);

/* ---- walk ---------------------------------------------------------------------------------- */
typedef struct {
  float p, q;          /* --p / --q already cast to float (RandomWalk.scala:112) */
  int32_t walk_length; /* --walkLength: a full path has walk_length + 2 ids */
  int32_t num_walks;   /* --numWalks walk iterations in this call */
  int32_t first_walk;  /* index of the first walk iteration (Philox counter word 0) */
  int32_t rng_mode;    /* SRW_RNG_* */
  float const_r;
  uint32_t seed;
  int32_t sampler;     /* SRW_SAMPLER_* */
  int32_t flags;       /* SRW_WALK_* */
} srw_walk_params;
enum {
  SRW_WALK_FORCE_GENERAL = 1, /* use the general second-order kernel even when p == q == 1 (testing) */
  SRW_WALK_NT_LOADS = 2,      /* first-order kernel: force L1-bypassing (nontemporal) record loads */
  SRW_WALK_CACHED_LOADS = 4,  /* first-order kernel: force default-policy loads (default: chosen from the table size) */
  SRW_WALK_LEGACY_FLUSH = 8,  /* first-order kernel: flush the path tile every 16 steps from the row's start (A/B: tools/first_order_ab.py --arm flush) */
  SRW_WALK_NO_COMPACT = 16,   /* first-order kernel: do not use the 16-byte lattice records even when available */
  SRW_WALK_NO_PREFIX = 32,    /* general kernel: always stream N(curr); do not use the exact prefix-sum search */
  SRW_WALK_NO_EDGE_HASH = 64, /* Mode A: membership by binary search in the sorted rows instead of the edge hash set */
  SRW_WALK_NO_BINNED = 128,   /* Mode R, q != 1: never use the binned prefix-sum search (streaming scan instead) */
  SRW_WALK_DEVICE_FORMAT = 131072, /* srw_walk_and_save: the GPU formats the path text (path_format.hip); the host only writes it */
  SRW_WALK_NO_HUB_BITMAPS = 65536, /* Mode R, q != 1: do not build / use the hub rows' neighbor-set bitmaps */
  SRW_WALK_NO_EDGE_TABLES = 262144, /* Mode R, q != 1: do not build / use the per-edge bias tables */
  SRW_WALK_EDGE_TABLES_ALL = 524288 /* test switch: a table for EVERY certified pair, chunks of 4 candidates */
  /* bits 12-14: test switch, force the binned search's membership strategy (1 = P1, 2 = P2, 3 = id-window,
     4 = hub bitmap where there is one); bit 15: test switch, binned search and hub bitmaps on rows of any degree
     (defaults: degree >= 128, hubs of degree >= 1024) */
};

typedef struct {
  int64_t n_walkers;    /* num_walks * nVertices */
  int64_t n_steps;      /* sum over paths of (len - 1): the metric's unit */
  int64_t dead_ends;    /* "Zero Neighbors" accumulator, RandomWalk.scala:117 */
  int64_t sum_deg_curr; /* general kernel: sum of deg(curr) over steps (algorithmic bytes) */
  int64_t sum_deg_prev; /* general kernel: sum of deg(prev) over second-order steps with q != 1 */
  int64_t ent_reads;    /* first-order / alias kernels: table records read; general kernel: steps served by the prefix search */
  int64_t fallbacks;    /* steps that needed the exact sequential fallback */
  int64_t trials;       /* Mode A: alias draws (accepted + rejected) */
  double kernel_ms;     /* hipEvent time of the walk kernels of this call, on the handle's stream */
  int32_t kernel_kind;  /* 1 = first-order guide-table kernel, 2 = general second-order kernel, 3 = alias, 4 = metapath */
  int32_t record_bytes; /* bytes of one sampling-table record read by this kernel (16 compact / 32 / 0) */
  int64_t strategy_steps[12]; /* general kernel: steps served by each sampler, indexed by SRW_STRAT_* */
  int64_t edge_tables;       /* per-edge bias tables in use by this call (0: none built) */
  int64_t edge_table_bytes;  /* HBM held by them */
  double setup_ms;           /* host wall time this call spent building sampling tables before the first kernel */
} srw_walk_stats;
enum { /* srw_walk_stats.strategy_steps: which sampler of the general (second-order) kernel served a step */
  SRW_STRAT_EDGE_TABLE = 0, /* precomputed per-edge bias table: search + one chunk */
  SRW_STRAT_P1 = 1,         /* binned search, N(prev) looked up in the sorted N(curr) */
  SRW_STRAT_P2 = 2,         /* binned search, candidates probed in the edge hash set / sorted N(prev) */
  SRW_STRAT_W = 3,          /* binned search, sorted-chunk intersection */
  SRW_STRAT_P3 = 4,         /* binned search, hub neighbor-set bitmap */
  SRW_STRAT_SCAN = 5,       /* certified streaming scan (small rows, rows without a certificate, first steps) */
  SRW_STRAT_PREFIX = 6,     /* q == 1: prefix-sum search with the return edges as a short list */
  SRW_STRAT_CHAIN = 7,      /* the reference's sequential f64 chain (irregular rows, draws on a CDF boundary) */
  SRW_STRAT_EDGE_MASK = 8,  /* precomputed per-edge membership mask (rows below 256 candidates): no lookup at all */
  SRW_STRAT_Q1_LANE = 9,    /* p != 1, q == 1: one walker per lane (first-order guide table + exact prefix sums + return edge) */
  SRW_STAT_HANDED_OVER = 10, /* not a sampler: WALKERS the per-edge-table / per-lane kernels handed to the general kernel (redone there) */
  SRW_STAT_TIES_RESOLVED = 11 /* not a sampler: of those, the walkers whose boundary draw the chain kernels resolved ahead of the redo (srw_walk) */
};

/* Replaces RandomWalk.randomWalk (M/algorithm/RandomWalk.scala:75-176) incl. initFirstStep (:51-66):
 * num_walks iterations, one walker per present vertex (ascending id), walker index =
 * iteration * nVertices + rank(vertex).  Paths stay in HBM as int32 [n_walkers][walk_length + 2]
 * (unused tail = -1) plus int32 lens[n_walkers]. */
int32_t srw_walk(srw_handle *h, const srw_walk_params *params, srw_walk_stats *stats);
/* The whole randomWalk loop with the results streamed to HOST buffers: iteration i's kernel runs while iteration
 * i-1's paths travel over PCIe on a second HIP stream (two device staging buffers).  paths is
 * [num_walks * nVertices][walk_length + 2], lens [num_walks * nVertices]; allocate them with srw_host_alloc
 * (pinned) for full PCIe rate — pageable buffers work but serialise.  Replaces RandomWalk.randomWalk returning
 * the union of all iterations' paths (M/algorithm/RandomWalk.scala:168,175). */
int32_t srw_walk_to_host(srw_handle *h, const srw_walk_params *params, int32_t *paths, int32_t *lens,
                         srw_walk_stats *stats);
/* Main.doRandomWalk fused (M/Main.scala:53-62: rw.execute() then rw.save(...)): walks num_walks iterations and
 * writes <output_dir>/path/part-* + _SUCCESS while streaming — iteration i's kernel and PCIe transfer overlap the host's
 * formatting of iteration i-1 (pinned ring of two slices); the paths are never held as a whole in host memory.
 * With SRW_WALK_DEVICE_FORMAT in params->flags the GPU formats the text and the host only copies it out and writes it.
 * dead_ends_per_iteration (optional, [num_walks]) receives the reference's per-iteration "Zero Neighbors" count.
 * Fails with SRW_ERR_EXISTS before any work if <output_dir>/path exists. */
int32_t srw_walk_and_save(srw_handle *h, const srw_walk_params *params, const char *output_dir, int32_t n_parts,
                          int32_t write_crc, srw_walk_stats *stats, int64_t *dead_ends_per_iteration);
/* ---- walks from a list of start vertices (whole-graph handles) --------------------------------
 * No reference counterpart: RandomWalk.randomWalk always seeds one walker per vertex (initFirstStep, RandomWalk.scala:51-66).
 * Walk from these vertices instead of from every present vertex.  ids[n] (host) are vertex ids as the input
 * spelled them, in any order, duplicates allowed; the list is copied.  Until srw_clear_sources or the next
 * graph load, srw_walk / srw_walk_to_host / srw_walk_and_save seed num_walks * n walkers:
 * walker index = iteration * n + position in the list — every buffer size and output order documented above in
 * terms of nVertices / rank(vertex) then reads n / position in the list (iteration major, then LIST order).  A draw is
 * keyed by (seed, iteration, source id, step), never by the walker's index: the path of (iteration, v) is the very row the
 * full walk produces for it, and a duplicate entry repeats its path.  n == 0 is a valid list (zero walkers).  Which sampling
 * tables a call builds does not depend on the list (SRW_WALK_NO_EDGE_TABLES / _NO_HUB_BITMAPS give a cheap cold start).
 * SRW_ERR_INVALID, with the handle's previous list (or none) left in force, if an id is not a vertex of the
 * loaded graph (the message names the first such id and its position), if no graph is loaded, on a sharded
 * handle (world > 1) or while population 1 is selected.  A vertex of the graph is what srw_graph_vertices lists:
 * one that only appears as the destination of a directed edge is a vertex (its walk is the one-entry path).
 * The srw_shard_* family ignores the list; a cluster carries one of its own (srw_cluster_set_sources, below): a single shard
 * can neither check a list (it knows its own vertices only) nor commit it together with the others. */
int32_t srw_set_sources(srw_handle *h, const int32_t *ids, int64_t n);
/* The same with the ids already in device memory on the handle's GPU (a tensor of a training loop): copied and
 * checked on the handle's stream — the caller has made sure that the ids are written before the call; one 8-byte
 * read-back reports an unknown id. */
int32_t srw_set_sources_device(srw_handle *h, const void *d_ids, int64_t n);
int32_t srw_clear_sources(srw_handle *h);
/* *n = length of the list in force, -1 when there is none (walks start from every vertex). */
int32_t srw_sources(const srw_handle *h, int64_t *n);

/* ---- metapath walks: steps restricted to vertex types (whole-graph handles) ------------
 * No reference counterpart (the reference walks homogeneous graphs); the semantics are those of StellarGraph's
 * UniformRandomMetaPathWalk and PyG's MetaPath2Vec, with RandomSample.sample as the draw: the vertex at path position j must
 * have the type the pattern names for j.
 *
 * Vertex types.  One uint8 per present vertex, indexed by position in V, the ascending list srw_graph_vertices returns (as the
 * negative weights and the SGNS tables are).  d_types: n bytes in device memory on the handle's GPU; the bytes are copied on the
 * handle's stream (with them the type of every adjacency entry's vertex is laid out beside the rows, 1 byte per entry), the call
 * is complete on return.  d_types == NULL clears the types (n is ignored).  Loading a graph drops them.  SRW_ERR_INVALID, with
 * the previous types left in force: no graph loaded, n != nV, a NULL h, a sharded handle (world > 1), population 1 selected.
 * SRW_ERR_NOMEM, likewise with the previous types in force, when the per-entry bytes do not fit: the walk has no other sampler. */
int32_t srw_vertex_types_set(srw_handle *h, const void *d_types, int64_t n);
/* *n = nV when types are in force, -1 when there are none. */
int32_t srw_vertex_types(const srw_handle *h, int64_t *n);
/* The walk.  pattern[m] (host), 1 <= m <= 64, each entry in 0 .. 255 (a type) or -1 (any type).  Path position j (j = 0 is the
 * source) has the required type pattern[j mod m]: StellarGraph's metapath [a, p, a] is pattern = {a, p}.  Walkers, iterations,
 * first_walk, the start list of srw_set_sources and the result buffers are exactly srw_walk's: int32 [n_walkers][walk_length + 2]
 * with tail -1, plus lens.  The result replaces the handle's last walk result: srw_fetch_paths, srw_device_paths, srw_write_paths,
 * srw_skipgram_windows / _batch, srw_path_vertex_counts and srw_w2v_fit_device with NULL pointers then act on it.
 * A source whose type does not match pattern[0] yields the one-entry path [src].  Step s = 1 .. walk_length + 1:
 *   u           the very draw srw_walk uses for step s of that walker: draw_uniform(rng, iteration, source id as the input spelled
 *               it, s) — the Philox stream above, or const_r under SRW_RNG_CONST.
 *   candidates  the entries of N(curr) IN ROW ORDER whose vertex matches pattern[s mod m]; multi-edges and self-loops are kept (a
 *               self-loop's type is curr's own).  With no such entry (an empty row included) the walk ends.
 *   next        RandomSample.sample (M/algorithm/RandomSample.scala:12-25) applied to THAT SUBLIST with its raw weights: S = the
 *               f64 left fold of the sublist's weights, acc += (double)w / S entry by entry, the answer is the first entry with
 *               acc >= (double)u, and the sublist's HEAD if there is none.  An entry that does not match is no candidate — it is
 *               not a candidate of weight zero: it can be neither the first acc >= u (u = 0) nor the head.
 * The step is first-order only: p and q must both be 1.0f.
 * Two consequences: with pattern = {-1} the result is bit for bit srw_walk's with p = q = 1, for any types and any rng mode; and
 * so it is with every vertex of type t and pattern = {t}.
 * stats: n_walkers; n_steps = sum of (len - 1); dead_ends = walkers that stopped at a step s > 1 (the general kernel's rule: a
 * source of the wrong type or without a candidate at s = 1 is not counted); fallbacks = steps decided by the exact sequential
 * chain; kernel_ms; kernel_kind = 4; everything else 0.
 * SRW_ERR_INVALID before any launch, the previous walk result intact: a NULL h, params or pattern; no graph; a sharded handle
 * (world > 1); population 1 selected; no types in force (even for an all-wildcard pattern); m outside 1 .. 64; an entry outside
 * -1 .. 255; p != 1 or q != 1; sampler != SRW_SAMPLER_REFERENCE; whatever srw_walk refuses in walk_length, num_walks or rng_mode.
 * params->flags is ignored. */
int32_t srw_walk_metapath(srw_handle *h, const srw_walk_params *params, const int32_t *pattern, int32_t m, srw_walk_stats *stats);

/* ---- neighbour sampling: the layered fan-out sample of a mini-batch of seeds (whole-graph handles) ------------
 * No reference counterpart (the reference only walks); the semantics are those of StellarGraph's SampledBreadthFirstWalk and of the
 * sampler behind PyG's NeighborLoader / DGL's sample_neighbors, with RandomSample.sample as the weighted draw.  It reads the tables a
 * p = q = 1 srw_walk builds and nothing else.
 *
 * Layout.  F_0 = 1 and F_l = F_{l-1} * fanouts[l-1].  Layer l (1-based, l = 1 .. n_layers) is int32 [n_seeds][F_l], row-major, written to
 * d_layers[l-1] (the caller's buffers, device memory on the handle's GPU); layer 0 is the seed list d_seeds [n_seeds].  The parent of
 * element (b, j) of layer l is element (b, j / fanouts[l-1]) of layer l-1.  The tree's edges are implicit in the positions: layer l
 * viewed as [n_seeds][F_{l-1}][fanouts[l-1]] groups the children by parent — the form GraphSAGE's mean aggregator consumes.  No
 * relabelling and no edge list are produced; a deduplicated subgraph with a relabelled edge_index is out of scope.
 *
 * Ids are the input's ids, also on a graph with compacted ids, as in every other tensor entry point.  An element is -1 when its parent
 * is -1, when its parent is no present vertex of the graph (below the smallest or above the largest id, in a gap), or when its
 * parent's row is empty (a dead end, or a destination-only vertex of a directed graph): the whole subtree below a -1 is -1.  -1 is the
 * padding value and never names a vertex here, not even on a graph that holds a vertex -1.  *n_unknown counts the SEEDS that are no
 * present vertex, -1 included (deeper layers hold only -1 or ids the graph itself supplied).  No id reaches an address before
 * device_common.h:vertex_slot has checked it, so no tensor content can send a load or a store outside a table.
 *
 * The draw of element (b, j) of layer l:  word = philox4x32_10(ctr = (b, j, l, epoch), key = (seed, 64))[0].  b is the seed's index
 * WITHIN THE CALL, never the vertex id: a vertex that occurs twice gets independent children, and a seed's subtree does not depend on
 * what else is in the batch.  Key words 0 .. 32 are taken by the walk and the negatives; 64 is this stream's.
 *   replace != 0   (StellarGraph's semantics, and the reference's draw)  m = word >> 8, u = m * 2^-24; the element is the entry that
 *                  RandomSample.sample (M/algorithm/RandomSample.scala:12-25) returns for N(parent) with its raw weights and u — exactly
 *                  what step 1 of srw_walk does with its own u: S = the f64 left fold of the weights, acc += (double)w / S entry by
 *                  entry, the first entry with acc >= (double)u, the row's head if there is none.  Multi-edges and self-loops are
 *                  entries like any other.  The 24-bit lattice has the same consequence as for the walk: of a row beyond 2^24 entries
 *                  some can never be drawn.
 *   replace == 0   (PyG's / DGL's default)  uniform over the row's ENTRIES — positions in srw_graph_neighbors order —, ignoring the
 *                  weights, without repeating a position.  With deg = |N(parent)| and f = fanouts[l-1]: if deg <= f the children are
 *                  the row's entries in row order, then -1.  Otherwise Floyd's algorithm in selection order, for i = 0 .. f-1:
 *                  J = deg - f + i, t = (uint64(word_i) * (J + 1)) >> 32 with word_i the word of the child's own output position
 *                  j = jp * f + i (jp the parent's position in its row of layer l-1); child i is entry t of the row if no earlier
 *                  child of this parent took position t, else entry J.  Positions are distinct; ids may repeat on a multi-graph.
 *
 * The call runs on the handle's stream, one launch per layer (layer l reads layer l-1), and is complete on return; the unknown count
 * (8 bytes) is the only read-back; every offset is 64-bit (n_seeds * F_l may exceed 2^31).  The first-order tables are built on first
 * use, exactly as a p = q = 1 srw_walk would build them.  The handle's last walk result, sources, vertex types and negative weights
 * are untouched.  SRW_NBR_NO_COMPACT in flags is a test switch: draw through the 32-byte first-order records even where the compact
 * ones exist (the results are the same element for element).
 * SRW_ERR_INVALID before any launch, the outputs untouched: a NULL h / np / fanouts / d_layers; no graph loaded; a sharded handle
 * (world > 1); population 1 selected; n_layers outside 1 .. 8; a fanout outside 1 .. 4096; a fanout above 64 with replace == 0;
 * F_L >= 2^31 (L = n_layers); n_seeds < 0 or >= 2^31; flags with an unknown bit; then, for n_seeds > 0: a NULL d_seeds, a NULL layer
 * pointer, a pointer that is not 4-byte aligned, a layer's byte range overlapping the seeds' or another layer's.  n_seeds == 0 is
 * SRW_OK whatever the pointers are (an empty tensor's are arbitrary): nothing is launched, *n_unknown = 0. */
typedef struct { uint32_t seed; uint32_t epoch; int32_t replace; int32_t flags; } srw_neighbor_params;   /* 16 bytes */
enum { SRW_NBR_NO_COMPACT = 1 /* test switch: draw through the 32-byte first-order records even where the compact ones exist */ };
int32_t srw_sample_neighbors(srw_handle *h, const void *d_seeds /* int32 [n_seeds] */, int64_t n_seeds,
                             const int32_t *fanouts /* host, [n_layers] */, int32_t n_layers, const srw_neighbor_params *np,
                             void *const *d_layers /* host array of n_layers device pointers */, int64_t *n_unknown /* or NULL */);

/* Importance neighbours (importance.hip): PinSAGE's neighbourhood of a seed — the T vertices that R short random walks with
 * restart from it visit most often, with the visit counts as importance weights (DGL's PinSAGESampler / RandomWalkNeighborSampler; with a
 * long horizon the Monte-Carlo estimate of personalised PageRank).  No reference counterpart.  R = num_walks, L = walk_length, T = top.
 *
 * The walks.  Seed b is the seed's index WITHIN THE CALL, never the vertex id.  It runs walks w = 0 .. R-1, each of at most L steps
 * s = 0 .. L-1, and step s of walk w has  words = philox4x32_10(ctr = (base + b, w, s, epoch), key = (seed, 65)).  Key word 65 is this
 * stream's (0 .. 32 and 64 are taken).  base lets a long list be processed in several calls with the same result as one call: seed b of
 * a call with base = k gets exactly what seed k + b of a call with base = 0 gets.  The walk stands on curr, the seed at s = 0.  Before a
 * step s >= 1 the walk ends if (words[1] >> 8) < restart_m (restart_m in 0 .. 2^24: 0 means never, 2^24 means always — every walk is then
 * exactly one step; the first step is never cut).  The walk also ends if N(curr) is empty.  Otherwise m = words[0] >> 8, u = m * 2^-24,
 * and next is the entry that RandomSample.sample (M/algorithm/RandomSample.scala:12-25) returns for N(curr) with its raw weights and u —
 * step 1 of srw_walk, and srw_sample_neighbors with replace != 0, with another u, the 24-bit lattice included.  The walk is first-order
 * at every step: no p, no q, no previous vertex.  Arriving at next is one visit; then curr = next.
 *
 * The counts.  c(v) is the number of visits of v over the R walks of this seed.  Without SRW_IMP_KEEP_SEED the visits of the seed's own
 * vertex are dropped (the walk still passes through it).  d_total[b] is the sum of c(v) over all v, after that drop and before any
 * truncation: at most R * L.  The result row of b is the vertices with c(v) > 0 ordered by c descending, then by id ascending (the
 * input's id, as a signed int32); the first T of them go to d_ids[b] with their c in d_counts[b]; padding is id -1 with count 0.  Ids are
 * the input's ids, also on a graph with compacted ids.  A seed that is -1 or no present vertex gets an all-padding row and total 0 and is
 * counted in *n_unknown; a present seed with an empty row gets the same row and total 0 but is not counted.  A vertex that occurs twice
 * in the batch gets independent walks, and a seed's row does not depend on what else is in the batch.  Only the seed is an id a tensor
 * supplies: it reaches no address before device_common.h:vertex_slot has checked it; every later vertex is one the graph itself supplied.
 *
 * The call runs on the handle's stream and is complete on return; the unknown count (8 bytes) is the only read-back; every offset is
 * 64-bit.  The visits of a chunk of seeds are kept in a buffer of the handle of at most 1 GiB; more seeds than fit are processed chunk
 * after chunk on the stream.  The first-order tables are built on first use, exactly as a p = q = 1 srw_walk would build them.  The
 * handle's last walk result, sources, vertex types and negative weights are untouched.  SRW_IMP_NO_COMPACT is a test switch, as
 * SRW_NBR_NO_COMPACT (the results are the same element for element).
 * SRW_ERR_INVALID before any launch, the outputs untouched: a NULL h / ip; no graph loaded; a sharded handle (world > 1); population 1
 * selected; num_walks outside 1 .. 4096; walk_length outside 1 .. 4096; num_walks * walk_length > 4096; top outside 1 .. 64;
 * restart_m > 2^24; flags with an unknown bit; n_seeds < 0 or >= 2^31; base + n_seeds > 2^32; then, for n_seeds > 0: a NULL d_seeds /
 * d_ids / d_counts, a pointer that is not 4-byte aligned, any two of the four byte ranges (three when d_total is NULL) overlapping.
 * n_seeds == 0 is SRW_OK whatever the pointers are: nothing is launched, *n_unknown = 0. */
typedef struct { uint32_t seed; uint32_t epoch; uint32_t base; int32_t num_walks; int32_t walk_length;
                 int32_t top; uint32_t restart_m; int32_t flags; } srw_importance_params;   /* 32 bytes */
enum { SRW_IMP_KEEP_SEED = 1, SRW_IMP_NO_COMPACT = 2 /* test switch, as SRW_NBR_NO_COMPACT */ };
int32_t srw_importance_neighbors(srw_handle *h, const void *d_seeds /* int32 [n_seeds] */, int64_t n_seeds,
                                 const srw_importance_params *ip, void *d_ids /* int32 [n_seeds][top] */,
                                 void *d_counts /* int32 [n_seeds][top] */, void *d_total /* int32 [n_seeds], or NULL */,
                                 int64_t *n_unknown /* or NULL */);

/* Pinned (page-locked) host memory for srw_walk_to_host / srw_fetch_paths destinations. */
int32_t srw_host_alloc(size_t bytes, void **out);
void srw_host_free(void *p);
/* Copy the last walk's paths / lens to host buffers (either may be NULL). */
int32_t srw_fetch_paths(const srw_handle *h, int32_t *paths, int32_t *lens);
/* Device pointers of the last walk's result (valid until the next srw_walk / destroy). */
int32_t srw_device_paths(const srw_handle *h, void **d_paths, void **d_lens, int64_t *n_walkers, int32_t *stride);
/* Replaces RandomWalk.save (M/algorithm/RandomWalk.scala:234-241) + Property.pathSuffix: writes
 * <output_dir>/path/part-00000.. (TAB-joined ids, one '\n' per path) and _SUCCESS; canonical line
 * order (walk iteration major, source id ascending; after srw_set_sources: iteration major, then list order).
 * write_crc != 0 adds Hadoop .crc side files.
 * The text is formatted on the GPU from the device-resident result (SRW_HOST_FORMATTER=1: on host threads). */
int32_t srw_write_paths(const srw_handle *h, const char *output_dir, int32_t n_parts, int32_t write_crc);

/* Mode A table of vertex v (build-defined exact-integer alias construction): prob/alias of each
 * neighbor slot (alias = position inside the row); *regular = 0 when the row is not alias-regular (Mode A
 * then samples it by CDF inversion).  *n as srw_graph_neighbors. */
int32_t srw_alias_row(srw_handle *h, int32_t v, float *prob, int32_t *alias, int64_t cap, int64_t *n, int32_t *regular);

/* ---- vertex-sharded multi-GPU path (one handle per GPU, world > 1) -------------------------- */
/* Replaces the Spark shuffle of the super-step loop: prepareWalkersToTransfer (UniformRandomWalk.scala:103-112,
 * VCutRandomWalk.scala:121-134) + transferWalkersToTheirPartitions (RandomWalk.scala:186-192) + the loop itself
 * (RandomWalk.scala:91-162).  The graph is sharded by source vertex (srw_config.rank / world); a walker standing on v is
 * processed by owner(v); its PATH stays on its home rank = owner(source).  Each super-step every rank consumes one
 * receive buffer of `world` fixed-capacity chunks (one per sender) and fills `world` destination chunks:
 *     chunk = { uint32 n_walkers, n_rets, 0, 0 } | srw_walker[cap_walkers] | srw_path_ret[cap_rets]
 * — 16 + 8 = 24 bytes per walker-step on the wire (the reference ships the path so far and N(prev), RandomWalk.scala:135).
 * The caller moves chunk (me -> d) to rank d's receive buffer slot `me`: one equal-split all-to-all of chunk_bytes per
 * peer (RCCL over xGMI; stellar-random-walk_amd/distributed.py), or — one process, several devices — the kernels store
 * straight into the peers' receive buffers (srw_cluster_*, below).  No host synchronisation per super-step: counts live
 * in the chunk headers; an overflowing chunk drops its surplus and srw_shard_finish reports it (retry with more slack).
 * The keyed RNG makes the paths bit-identical for any world size (tests assert it against the oracle). */
typedef struct {            /* 16 bytes on the wire */
  int32_t lw;               /* home rank's path row: local vertex index * batch + iteration in batch */
  int32_t src;              /* source vertex (Philox key; owner(src) = home rank) */
  int32_t prev, curr;       /* the walker stands on curr, came from prev (linked p = q = 1 walk: prev | curr << 32 = row link of the vertex it stands on) */
} srw_walker;
typedef struct {            /* 8 bytes: one path slot of walker lw, returned to its home rank; the slot is implicit — a return
                               produced by super-step s is slot s */
  int32_t lw;               /* top bit set: death notice (the walker stopped before sampling slot s: its path has s entries) */
  int32_t v;
} srw_path_ret;
typedef struct { int64_t cap_walkers, cap_rets, chunk_bytes; } srw_shard_layout;
/* vertices owned by this handle / present in the whole graph (the walker seeds, UniformRandomWalk.scala:81-87) */
int32_t srw_shard_capacity(const srw_handle *h, int64_t *n_local_vertices, int64_t *n_global_vertices);
/* global rank (position among all present vertices, ascending id) of each local vertex: path row lw of a batch of B
 * iterations is canonical walker (first_walk + lw % B) * nVertices + ranks[lw / B].  out[n_local_vertices] (host). */
int32_t srw_shard_vertex_ranks(const srw_handle *h, int32_t *out);
/* Chunk capacities for `batch` walk iterations sharing their super-steps: slack * batch * nVertices / world^2 + 4096. */
int32_t srw_shard_layout_for(const srw_handle *h, int32_t batch, double slack, srw_shard_layout *out);
/* Two walker populations per handle: population 0 (the default) and 1 each have their own super-step context (scratch, cursors,
 * counters, path staging) and their own stream; srw_shard_begin / _superstep / _flush / _finish act on the selected one.  A driver
 * that interleaves the super-steps of two populations lets one's kernels run while the other's chunks are being exchanged — the
 * overlap the reference's shuffle / count rhythm (RandomWalk.scala:91-162) does not have.  Select 0 again before any other call
 * on the handle: while population 1 is selected, srw_walk*, the loads, srw_w2v_fit* and srw_probe_request_rate fail with
 * SRW_ERR_INVALID (they would run on the second population's stream with its cursors); srw_set_stream sets the SELECTED
 * population's stream. */
int32_t srw_shard_select(srw_handle *h, int32_t population);
/* Seeds this rank's batch * n_local walkers into its own receive buffer d_recv (world * chunk_bytes, device), writes
 * path slot 0 / lens into d_paths [batch * n_local][walk_length + 2] / d_lens (device), clears the counters. */
int32_t srw_shard_begin(srw_handle *h, const srw_walk_params *params, int32_t batch, const srw_shard_layout *layout,
                        void *d_recv, void *d_paths, void *d_lens);
/* Super-step `step` (1 .. walk_length + 1), enqueued on the handle's stream: applies the path returns found in d_recv,
 * samples every walker in d_recv once, writes chunk (me -> d) to dst_chunks[d] (device or peer pointers, d < world). */
int32_t srw_shard_superstep(srw_handle *h, const srw_walk_params *params, int32_t batch, int32_t step,
                            const srw_shard_layout *layout, const void *d_recv, void *const *dst_chunks, void *d_paths,
                            void *d_lens);
/* After the exchange that follows super-step walk_length + 1: applies its path returns. */
int32_t srw_shard_flush(srw_handle *h, const srw_walk_params *params, int32_t batch, const srw_shard_layout *layout,
                        const void *d_recv, void *d_paths, void *d_lens);
/* Synchronises the stream; steps / dead ends since srw_shard_begin; *overflow != 0: a chunk was too small. */
int32_t srw_shard_finish(srw_handle *h, srw_walk_stats *stats, int32_t *overflow);
/* Device memory on the handle's GPU for callers without an allocator of their own (exchange buffers of the sharded
 * walk: one hipMalloc per buffer — RCCL faulted on multi-GB buffers that were sub-blocks of a caching allocator's
 * segment, profiles/r02i).  srw_device_free(h, NULL) is a no-op. */
int32_t srw_device_alloc(srw_handle *h, int64_t bytes, void **d_ptr);
int32_t srw_device_free(srw_handle *h, void *d_ptr);
/* Optional, once per loaded graph, before the first p = q = 1 walk: row descriptors across shards.  The replicated
 * first-order records carry the row descriptor of the neighbor they name, so a step never reads the row table; on a
 * shard that row lives on the neighbor's OWNER.  Each shard exports its row table (16 bytes per dense id slot:
 * int64 offset, int32 degree, uint32 flags; zeros for vertices it does not own), the tables are combined by an
 * element-wise maximum of their int64 words (an all-reduce MAX; inside one process srw_shard_rows_merge over peer
 * pointers), and srw_shard_rows_commit derives 16-byte records whose links point into the owners' tables.  The walkers
 * of a p = q = 1 Philox walk then travel with the link of the vertex they stand on (srw_walker.prev / kind hold it),
 * and sampling + bucketing run as one kernel.  EVERY shard must end up linked (*linked == 1) — if one does not (a
 * record needing an escape), call srw_shard_rows_release on all of them: the unlinked path keeps working. */
int32_t srw_shard_rows_count(const srw_handle *h, int64_t *n_slots);
int32_t srw_shard_rows_export(srw_handle *h, void *d_rows, int64_t n_slots);
int32_t srw_shard_rows_merge(srw_handle *h, void *d_rows, const void *d_other_rows, int64_t n_slots);
int32_t srw_shard_rows_commit(srw_handle *h, const void *d_rows_all, int64_t n_slots, int32_t *linked);
int32_t srw_shard_rows_release(srw_handle *h);

/* ---- the same walk inside ONE process over several devices (CLI --gpus N, the JNI host) ------------------------------ */
/* One sharded handle per device, peer access enabled; the bucket kernels store every chunk directly into the receiving
 * device's buffer over xGMI and the super-steps are ordered by events — no collective library, no host sync per step.
 * devices may repeat an ordinal (several shards on one GPU: how the protocol is tested on a single-GPU box). */
typedef struct srw_cluster srw_cluster;
int32_t srw_cluster_create(const int32_t *devices, int32_t n_devices, int32_t flags, srw_cluster **out);
void srw_cluster_destroy(srw_cluster *c);
const char *srw_cluster_last_error(const srw_cluster *c);
srw_handle *srw_cluster_shard(srw_cluster *c, int32_t rank);   /* the rank's handle (graph queries, tests) */
int32_t srw_cluster_load_edgelist(srw_cluster *c, const char *path, int32_t directed, int32_t weighted, int32_t partitioned,
                                  int32_t rdd_partitions);
int32_t srw_cluster_load_coo(srw_cluster *c, const int32_t *src, const int32_t *dst, const float *w, const int32_t *pid,
                             int64_t n_lines, int32_t directed);
int32_t srw_cluster_generate_rmat(srw_cluster *c, int32_t scale, int64_t n_edges, uint32_t seed, int32_t weighted, int32_t directed);
int32_t srw_cluster_graph_stats(const srw_cluster *c, int64_t *n_vertices, int64_t *n_entries);
/* params->num_walks iterations starting at first_walk, `batch` of them per population (0 = automatic); paths stay on
 * their home devices.  stats: n_steps / dead_ends summed over the shards, kernel_ms = wall time of the super-steps. */
int32_t srw_cluster_walk(srw_cluster *c, const srw_walk_params *params, int32_t batch, srw_walk_stats *stats);
/* The last walk in canonical order (iteration major, source id ascending): paths [num_walks * nVertices][walk_length + 2]
 * (after srw_cluster_set_sources: iteration major, then list order, [num_walks * n][walk_length + 2]). */
int32_t srw_cluster_fetch_paths(srw_cluster *c, int32_t *paths, int32_t *lens);
/* walk + RandomWalk.save (RandomWalk.scala:234-241) over the cluster: <output_dir>/path/part-* + _SUCCESS.  The job is streamed
 * batch by batch (device memory: one batch of paths per shard, host memory: one slice), so NO walk result stays behind:
 * srw_cluster_fetch_paths after this call fails with "no walk result" — use srw_cluster_walk when the paths are wanted in memory. */
int32_t srw_cluster_walk_and_save(srw_cluster *c, const srw_walk_params *params, const char *output_dir, int32_t n_parts,
                                  int32_t write_crc, srw_walk_stats *stats);
/* ---- walks from a list of start vertices on the cluster ---------------------------------------
 * srw_set_sources for the vertex-sharded walk, with its semantics: ids[n] (host) are vertex ids as the input spelled them, in any
 * order, duplicates allowed; the list is copied.  Until srw_cluster_clear_sources or the next srw_cluster_load_* /
 * _generate_rmat, srw_cluster_walk / _fetch_paths / _walk_and_save seed num_walks * n walkers: canonical walker = iteration * n +
 * position in the list (iteration major, then LIST order), stats.n_walkers = num_walks * n, and every buffer the caller sizes
 * reads n where it read nVertices.  The path of (iteration, v) is the row the full walk produces for it — for any world, on
 * repeated device ordinals as on distinct devices —, a duplicate entry repeats its path, n == 0 gives zero walkers and an empty
 * but complete <output>/path.  Which sampling tables a call builds does not depend on the list.
 * Every shard keeps the entries whose vertex it owns, in list order, with their positions (one HIP kernel + a stable
 * compaction per shard); chunk capacities are sized from n and from the list's skew over the ranks, and the overflow retry
 * stays behind them.  A set or a clear drops a held walk result (srw_cluster_fetch_paths then fails until the next walk).
 * SRW_ERR_INVALID, with the previous list (or none) left in force on EVERY shard, if an id is no vertex of the loaded graph —
 * what srw_graph_vertices of a whole-graph handle lists; a destination-only vertex of a directed graph is one — (the message
 * names the first such id and its position), if no graph is loaded, if c is NULL, n < 0 or n >= 2^31.
 * The multi-device path has run on virtual shards of one device only. */
int32_t srw_cluster_set_sources(srw_cluster *c, const int32_t *ids, int64_t n);
int32_t srw_cluster_clear_sources(srw_cluster *c);
/* *n = length of the list in force, -1 when there is none (walks start from every vertex). */
int32_t srw_cluster_sources(const srw_cluster *c, int64_t *n);

/* ---- the embedding stage (`--cmd node2vec` / `--cmd embedding`) ---------------------------------------
 * Replaces Main.configureWord2Vec + Word2Vec.fit + the vector part of saveModelAndFeatures (M/Main.scala:36-44,77-97,113-124):
 * skip-gram with hierarchical softmax over the paths, trained on the GPU (csrc/embedding.hip).  org.apache.spark.mllib.feature.
 * Word2Vec is a dependency that is absent from the reference tree and seeds itself from the clock: PARITY UNPINNED — the build
 * restates the published algorithm with a seed of its own and is checked against its CPU restatement (oracle: orc_w2v_fit). */
typedef struct {
  int32_t dim;            /* --dim     (setVectorSize)    */
  int32_t window;         /* --window  (setWindowSize)    */
  int32_t iterations;     /* --iter    (setNumIterations) */
  float learning_rate;    /* --lr      (setLearningRate)  */
  uint32_t seed;          /* the build's seed (MLlib: Utils.random.nextLong(), unseeded) */
  int32_t threads;        /* 1: one wave, sentences in order (the sequential form); anything else: one wave per sentence, Hogwild */
} srw_w2v_params;
/* paths [n][stride] / lens on the HOST (what srw_fetch_paths returns, or a parsed paths file).  Outputs are malloc'ed (srw_free):
 * vocab_ids[n_vocab] = the ids by descending count (ties: ascending id; minCount 0), vectors[n_vocab * dim]. */
int32_t srw_w2v_fit(srw_handle *h, const int32_t *paths, const int32_t *lens, int64_t n, int64_t stride, const srw_w2v_params *params,
                    int32_t **vocab_ids, float **vectors, int64_t *n_vocab);
/* The same with the paths where srw_walk left them: in HBM (d_paths [n][stride], d_lens [n]: what srw_device_paths returns; both NULL =
 * this handle's last walk result).  This is the reference's hand-over — `randomWalk(...)` feeds Word2Vec.fit without leaving the
 * cluster (M/Main.scala:113-117): tokens are flattened, sorted, run-length encoded and ranked on the device; only the vocabulary's counts
 * (for the Huffman tree) and the trained vectors cross PCIe. */
int32_t srw_w2v_fit_device(srw_handle *h, const void *d_paths, const void *d_lens, int64_t n, int64_t stride, const srw_w2v_params *params,
                           int32_t **vocab_ids, float **vectors, int64_t *n_vocab);
/* ---- skip-gram training batches (no reference counterpart: the reference's trainer is MLlib's hierarchical softmax, above) --------
 * What a negative-sampling loss over someone's own embedding table consumes, built on the device from paths in the layout srw_walk
 * leaves them (d_paths [n][stride] int32, row r = lens[r] ids then -1; d_lens [n], 1 <= lens[r] <= stride; both NULL = this handle's
 * last walk result, n and stride then come from it):
 *   pos [W][context]        every run of `context` consecutive vertices of every path.  Row r has cnt[r] = max(0, lens[r] - context + 1)
 *                           windows, window (r, j) = paths[r][j .. j + context - 1] is output row off[r] + j, off = exclusive prefix sum
 *                           of cnt (row-major, then j ascending), W = sum of cnt.  No window holds a -1.
 *   neg [W][num_negatives]  entry k of window (r, j) = V[(word * nV) >> 32] with
 *                           word = philox4x32_10(ctr = (r, j, k >> 2, epoch), key = (seed, 1))[k & 3] and V[nV] the present vertices in
 *                           ascending order (what srw_graph_vertices lists; input ids, also on a graph whose ids were compacted).
 *                           Uniform over the present vertices and NOT filtered against the window's own vertices (as PyG's
 *                           Node2Vec.neg_sample).  The key is (row index WITHIN THE CALL, window start, k), never the window's place in
 *                           the output: a row's negatives do not depend on what else is in the batch, and a call over rows [a, b) of a
 *                           result (pointer offset, n = b - a) keys row r of the result as r - a.  Key word 1 keeps the stream apart
 *                           from the walk's (seed, 0); epoch gives fresh negatives for the same rows on the next pass.
 * d_pos == NULL: count only — *n_windows = W, nothing else is written (one reduction over lens).  Otherwise d_pos[W * context] and, when
 * num_negatives > 0, d_neg[W * num_negatives] (the caller's buffers, int32, 4-byte aligned) are filled, unless W > cap_windows: then
 * nothing is written, *n_windows = W and the call fails with SRW_ERR_INVALID (the message names both numbers).  The work runs on the
 * handle's stream and is complete on return; W (8 bytes) is the only read-back.  Every offset is 64-bit: W * context may exceed 2^31.
 * SRW_ERR_INVALID before anything is launched: a NULL h / sp / n_windows, no walk result behind NULL pointers (or one pointer alone),
 * n < 0 or n, stride >= 2^31, context < 1 or > stride, num_negatives < 0, num_negatives > 0 with no graph loaded or (when filling)
 * without d_neg, a sharded handle (world > 1), population 1 selected.  n == 0 and W == 0 are valid results; context == 1 is valid.
 * n == 0 with a pointer given is SRW_OK with *n_windows = 0 whatever stride and the other pointer are (an empty tensor's are arbitrary);
 * two NULL pointers always mean the last walk result, never an empty array. */
typedef struct { int32_t context; int32_t num_negatives; uint32_t seed; uint32_t epoch; } srw_skipgram_params;
int32_t srw_skipgram_windows(srw_handle *h, const void *d_paths, const void *d_lens, int64_t n, int64_t stride,
                             const srw_skipgram_params *sp, void *d_pos, void *d_neg, int64_t cap_windows,
                             int64_t *n_windows);
/* ---- negatives by vertex weight, kept out of their own window (single-GPU handles) ---------------------------------------
 * V[nV] is the ascending list of present vertices that srw_graph_vertices returns; every weight and count below is indexed by position
 * in V.  All four entries are SRW_ERR_INVALID on a NULL handle, a sharded handle (world > 1) or while population 1 is selected; they
 * run on the handle's stream and are complete on return; argument errors come before any launch; every offset is 64-bit.
 *
 * Weight table.  d_w: n unsigned 32-bit weights in device memory on the handle's GPU.  cdf[i] = w[0] + ... + w[i] as uint64 and
 * T = cdf[nV - 1].  SRW_ERR_INVALID, with the previous table left in force: n != nV, T == 0, no graph loaded (or one without a vertex),
 * a pointer that is not aligned to 4 bytes.  d_w == NULL clears the table (n is ignored): draws are uniform again.  Loading a graph
 * drops the table. */
int32_t srw_negative_weights_set(srw_handle *h, const void *d_w, int64_t n);
/* d_out (device memory) receives nV int64 values: the row length of V[i] — what srw_graph_neighbors reports in *n; 0 for a
 * destination-only vertex of a directed graph. */
int32_t srw_graph_degrees_device(srw_handle *h, void *d_out);
/* d_counts (device memory) receives nV int64 values: how often V[i] occurs in the first lens[r] entries of the rows of d_paths
 * [n][stride] / d_lens [n] (int32, device memory; both NULL = this handle's last walk result, n and stride then come from it).  A
 * length above the stride is read as the stride.  An id that is no vertex of the graph (only a caller's own arrays can hold one) is
 * counted in *n_unknown and nowhere else.  d_counts is overwritten, not accumulated; n == 0 with a pointer given zeroes it.
 * SRW_ERR_INVALID: no graph loaded, NULL d_counts / n_unknown, no walk result behind NULL pointers (or one pointer alone), n < 0 or
 * n, stride >= 2^31, stride < 1. */
int32_t srw_path_vertex_counts(srw_handle *h, const void *d_paths, const void *d_lens, int64_t n, int64_t stride, void *d_counts,
                               int64_t *n_unknown);
/* srw_skipgram_windows with negatives by the weight table in force and, optionally, none that repeats a vertex of its own window.
 * Windows, pos, the count-only form (d_pos == NULL), cap_windows and the argument errors are exactly those of srw_skipgram_windows (the
 * same scan and the same fill kernel write pos).  neg [W][num_negatives]: entry k of window (r, j), attempt a (a = 0 when nothing is
 * excluded), r the row index within the call and j the window start as above:
 *   with a table    blk = philox4x32_10(ctr = (r, j, k >> 1, epoch), key = (seed, 2 + 2 a)),
 *                   u = (uint64(blk[2 (k & 1)]) << 32) | blk[2 (k & 1) + 1],  t = (u * T) >> 64 (the high half of the 128-bit product),
 *                   i = the smallest index with cdf[i] > t; the negative is V[i] (the input id, also on a graph with compacted ids).
 *                   A vertex of weight 0 is never drawn.
 *   without one     V[(word * nV) >> 32], word = philox4x32_10(ctr = (r, j, k >> 2, epoch), key = (seed, 1 + 2 a))[k & 3]: attempt 0 is
 *                   srw_skipgram_windows' draw.  Odd key words are uniform, even ones weighted; the walk keeps (seed, 0).
 * exclude_window != 0: a draw equal to any of the `context` vertices of its window is rejected and attempt a + 1 is taken, up to
 * max_draws attempts (1 .. 16, else SRW_ERR_INVALID; ignored when exclude_window == 0).  If every attempt is rejected,
 * the last attempt's vertex stands — not an error: a graph whose positive-weight vertices all lie in the window cannot do better.  With no table and
 * exclude_window == 0 the output is bit-identical to srw_skipgram_windows'. */
typedef struct { int32_t context; int32_t num_negatives; uint32_t seed; uint32_t epoch; int32_t exclude_window; int32_t max_draws; } srw_skipgram_batch_params;
int32_t srw_skipgram_batch(srw_handle *h, const void *d_paths, const void *d_lens, int64_t n, int64_t stride,
                           const srw_skipgram_batch_params *bp, void *d_pos, void *d_neg, int64_t cap_windows,
                           int64_t *n_windows);
/* ---- the negative-sampling training step over those batches (single-GPU handles) ------------------------------------------
 * What consumes pos [W][context] / neg [W][num_negatives]: one step of skip-gram with negative sampling on the CALLER's two embedding
 * tables, float32 [nV][dim], row-major, in device memory on the handle's GPU.  Rows are indexed by position in V (the ascending list
 * srw_graph_vertices returns), as the weights and counts above are; pos and neg hold vertex ids exactly as srw_skipgram_windows /
 * srw_skipgram_batch write them (the input ids, also on a graph with compacted ids); slot(id) is the id's position in V.
 * For window w:
 *   c      = slot(pos[w][center]), 0 <= center < context (0: the first vertex of the window is the centre, as PyG's Node2Vec samples;
 *            context / 2: the symmetric window)
 *   t_i    = the other context - 1 entries of pos[w], in order, with label 1, then the num_negatives entries of neg[w], with label 0
 *   f_i    = sum_d in[c][d] * out[t_i][d]
 *   g_i    = label_i - sigma(f_i)
 *   out_new[t_i][:] += lr * g_i * in[c][:]              for every i
 *   in_new[c][:]    += lr * sum_i g_i * out[t_i][:]
 *   loss[w] = sum_i softplus(-f_i) (label 1) or softplus(+f_i) (label 0), softplus(x) = log(1 + e^x), evaluated in a form that stays
 *            finite for any finite f.
 * There is NO clamp of f to +-6 and NO sigmoid table: this deliberately differs from word2vec.c (and from srw_w2v_fit above, which
 * restates it) — sigma and softplus are evaluated for the f that was computed, so that every output element can be held against a
 * float64 restatement of the lines above (tests/sgns_ref.py).
 * Every READ is from the old tables d_in / d_out, every ADD goes into the new tables.  Duplicates are simply more terms: a negative
 * equal to a context vertex, the same target twice, a target equal to the centre when one table serves both roles.
 *   exact step     d_in_new / d_out_new are separate buffers the caller initialised — clones of the old tables (the synchronous
 *                  mini-batch step) or zeros (with lr = -1 they then receive dLoss/d in and dLoss/d out, Loss = sum_w loss[w]).  The
 *                  result is a sum of well-defined terms and depends on the order of the additions only (float atomics: the last
 *                  bits may differ from run to run).
 *   in place       d_in_new == d_out_new == NULL: the adds go into d_in / d_out themselves (Hogwild).  Where no table row is named
 *                  twice in the whole call the result is the exact step's; where rows repeat, which value a read sees is unspecified,
 *                  as in word2vec.c across threads.  No add is lost: the adds are float atomics.
 * d_in == d_out is allowed (one table for both roles, as PyG's Node2Vec); then d_in_new == d_out_new is required.  Passing the old
 * table's own address as its new table is the in-place form of that table.  Any other overlap between the byte ranges of two of the
 * four tables, and any overlap of d_loss with one of them, is SRW_ERR_INVALID.
 * A window that holds an id which is no present vertex of the graph (below the smallest or above the largest id, in a gap, -1) is
 * skipped whole: it makes no add, its loss[w] is 0 and it is counted in *n_skipped.  No id reaches an address before its position has
 * been checked against nV, so no tensor content can send a store outside a table.
 * d_loss: float32 [n_windows] in device memory, overwritten, or NULL.  n_skipped may be NULL.  The call runs on the handle's stream and
 * is complete on return; the skip count (8 bytes) is the only read-back.  Every offset is 64-bit.
 * SRW_ERR_INVALID before anything is launched, the tables untouched: a NULL h / sp; no graph loaded, a sharded handle (world > 1),
 * population 1 selected; n_rows != nV; dim not a multiple of 64 in 64 .. 512; context < 1, num_negatives < 0, context + num_negatives
 * < 2 or > 64; center outside [0, context); a non-finite lr; reserved != 0; n_windows < 0; then, for n_windows > 0: a NULL d_pos /
 * d_in / d_out; num_negatives > 0 with d_neg == NULL; exactly one of d_in_new / d_out_new NULL; a pointer that is not aligned to 4
 * bytes; the overlap rules above.  n_windows == 0 is SRW_OK whatever the pointers are (an empty tensor's are arbitrary): nothing is
 * launched, *n_skipped = 0. */
typedef struct { int32_t context; int32_t num_negatives; int32_t dim; int32_t center; float lr; int32_t reserved; } srw_sgns_params;   /* 24 bytes */
int32_t srw_sgns_step(srw_handle *h, const void *d_pos, const void *d_neg, int64_t n_windows, const srw_sgns_params *sp,
                      const void *d_in, const void *d_out, void *d_in_new, void *d_out_new, int64_t n_rows,
                      void *d_loss /* float32 [n_windows] or NULL */, int64_t *n_skipped /* or NULL */);
/* ---- asking a table of vectors: the k nearest rows ---------------------------------------------------------------------------
 * srw_topk_rows: for each of n_queries queries the k best rows of d_table (float32 [n_rows][dim], row-major, device memory on the handle's
 * GPU), by cosine or by dot product, in ROW space: a table srw_sgns_step trained is in the order of V, srw_w2v_fit's vectors are in
 * vocabulary order; the search knows neither.  It needs no graph and works on any handle.  The n_queries x n_rows scores are never
 * formed: the table is read once per pass of up to 32 queries (16 for dim > 256, 8 for dim > 512).
 * Query forms.
 *   d_qrow only    query i is table row qrow[i], and that row is excluded from its own result (MLlib's findSynonyms(word)).  A qrow[i]
 *                  outside [0, n_rows) skips the query: its output row is padding and it is counted in *n_skipped.
 *   d_qvec only    query i is the vector qvec[i][0 .. dim) and nothing is excluded.
 *   both           the vector is the query and row qrow[i] is excluded; -1 means none; any other value outside [0, n_rows) skips the
 *                  query as above.
 *   neither        SRW_ERR_INVALID when n_queries > 0.
 * metric 1, dot:    score = sum_d q[d] r[d].
 * metric 0, cosine: score = dot / (sqrtf(sum q^2) * sqrtf(sum r^2)) with correctly rounded sqrt and divide; the score is exactly 0 when
 *                  either sum of squares is 0 (as MLlib; a table that starts at zero has such rows).  The row's sum of squares is taken
 *                  in the same pass, from the row the dot product reads: there is no array of norms to keep in step with the table.
 * Arithmetic: float32, every sum an fmaf chain over d = 0, 1, ..., dim - 1 starting from 0.  The score of (query, row) depends on those
 * two vectors alone — not on the row's position in the table, on n_queries, on k, or on which other queries share a pass — so identical
 * rows get identical score bits and a call repeats bit for bit.  A NaN score ranks, and is returned, as -inf; a score of -0 ranks, and is
 * returned, as +0.  Inputs whose sums of squares overflow float32 (or whose product of norms underflows to 0) are the caller's problem:
 * the scores are then whatever inf and NaN make of the formula above.
 * Order: the k best eligible rows by (score descending, row ascending) — a total order — in that order.  If fewer than k rows are
 * eligible the tail is padding: row -1, score -inf.  d_rows int32 [n_queries][k], d_scores float32 [n_queries][k], both overwritten.
 * No tensor content reaches an address unchecked: qrow[i] is compared with n_rows before it is multiplied into one.
 * The call runs on the handle's stream and is complete on return; the skip count (8 bytes) is the only read-back; n_skipped may be NULL.
 * Only 4-byte alignment is assumed of any pointer, and dim need not be a multiple of 4.  Every offset is 64-bit.
 * SRW_ERR_INVALID before anything is launched, the outputs untouched: a NULL h / tp; dim outside 1 .. 1024, k outside 1 .. 64, metric
 * not 0 or 1, reserved != 0; n_rows < 0 or >= 2^31, n_queries < 0; then, for n_queries > 0: a NULL d_table with n_rows > 0, a NULL
 * d_rows / d_scores, no query form, a pointer that is not aligned to 4 bytes, an output's byte range overlapping an input's or the other
 * output's.  n_queries == 0 is SRW_OK whatever the pointers are: nothing is launched, *n_skipped = 0.  n_rows == 0 with n_queries > 0
 * returns padding only (and, by row, skips every query). */
typedef struct { int32_t dim; int32_t k; int32_t metric; int32_t reserved; } srw_topk_params;   /* 16 bytes */
int32_t srw_topk_rows(srw_handle *h, const void *d_table /* float32 [n_rows][dim] */, int64_t n_rows,
                      const void *d_qvec /* float32 [n_queries][dim] or NULL */, const void *d_qrow /* int32 [n_queries] or NULL */,
                      int64_t n_queries, const srw_topk_params *tp,
                      void *d_rows /* int32 [n_queries][k] */, void *d_scores /* float32 [n_queries][k] */,
                      int64_t *n_skipped /* or NULL */);
/* Vertex ids to rows of such a table on the device: rows[i] = the position of ids[i] in V (the ascending list srw_graph_vertices
 * returns), -1 when the id is no vertex of the graph (below the smallest or above the largest id, in a gap); *n_unknown counts those.
 * ids are the input ids, also on a graph with compacted ids.  d_ids, d_rows: int32 [n] in device memory on the handle's GPU.
 * SRW_ERR_INVALID as srw_sgns_step: a NULL h, no graph loaded, a sharded handle (world > 1), population 1 selected, n < 0, and for n > 0
 * a NULL d_ids / d_rows or one that is not aligned to 4 bytes.  n == 0 is SRW_OK (*n_unknown = 0).  Complete on return. */
int32_t srw_vertex_rows(srw_handle *h, const void *d_ids /* int32 [n] */, int64_t n, void *d_rows /* int32 [n] */, int64_t *n_unknown /* or NULL */);
/* Unit-test hook (host only, no GPU): word2vec.c's CreateBinaryTree as the trainer uses it.  counts[n_vocab] in descending order ->
 * code_len[n_vocab], codes[n_vocab][40] (bits, root first), points[n_vocab][40] (rows of syn1 on the path, root = n_vocab - 2 first;
 * -1 beyond the code).  Known answers: tests/test_w2v_known_answers.py. */
int32_t srw_w2v_huffman(const int64_t *counts, int64_t n_vocab, int32_t *code_len, uint8_t *codes, int32_t *points);
/* "<id>\t<v0>\t...\t<v_dim-1>" lines (Main.scala:88-91; floats printed as java.lang.Float.toString prints them) into
 * <output_dir>/vec/part-%05d + _SUCCESS, and the model directory <output_dir>/bin as Word2VecModel.save lays it out: metadata/part-00000
 * (one JSON line) + data/part-00000.parquet — Parquet with Spark's schema for (word: String, vector: Array[Float]), written by
 * csrc/parquet_model.cpp (uncompressed; Spark writes snappy pages, any Parquet reader takes both).  As saveModelAndFeatures: the model first, then the vectors;
 * fails before writing anything if <output_dir>/bin or <output_dir>/vec exists, and removes what it created if it fails midway. */
int32_t srw_w2v_save(const int32_t *vocab_ids, const float *vectors, int64_t n_vocab, int32_t dim, const char *output_dir, int32_t n_parts);
/* The same for a vocabulary of WORDS (`--cmd embedding` on a text whose tokens are not vertex ids: the reference's Word2Vec takes any
 * token, M/Main.scala:119-124): words[r] is the NUL-terminated word of vocabulary row r. */
int32_t srw_w2v_save_words(const char *const *words, const float *vectors, int64_t n_vocab, int32_t dim, const char *output_dir, int32_t n_parts);

/* ---- measurement hooks (bench.py's `roofline` object; not on the walk's path) ------------------------ */
/* The ceiling the walk kernels are held against, measured on this handle's GPU in about a second: dependent, uniformly random
 * 16-byte reads (one chain per lane, 81 hops, the access pattern of a first-order step: one record per step) over a table of
 * `table_bytes` (0: 32 GiB; clipped to the free HBM).  *reads_per_s: reads = L2-miss requests per second; *table_gib (may be
 * NULL): the size actually used.  No reference counterpart: the reference has no device. */
int32_t srw_probe_request_rate(srw_handle *h, int64_t table_bytes, double *reads_per_s, double *table_gib);
/* What the REFERENCE's algorithm reads for the walk this handle just did (srw_walk; paths still resident), counted from the
 * finished paths: sums[0] = sum over the steps of deg(curr) (RandomSample.sample scans N(curr), RandomSample.scala:12-25),
 * sums[1] = sum over the second-order steps of deg(prev) (the `exists` over N(prev), RandomSample.scala:27-44), sums[2] = steps.
 * SURVEY §8(d)'s algorithmic bytes are 20 * sums[2] + 8 * sums[0] (+ 16 * second-order steps + 4 * sums[1] when q != 1). */
int32_t srw_result_scan_sums(srw_handle *h, int64_t *sums);

/* ---- unit hooks (device arithmetic of RandomSample, for parity tests) ----------------------- */
/* RandomSample.sample (M/algorithm/RandomSample.scala:12-25) on the GPU; *index = chosen position. */
int32_t srw_sample(srw_handle *h, const float *w, int64_t n, float r, int64_t *index);
/* RandomSample.computeSecondOrderWeights (:27-44) on the GPU. */
int32_t srw_second_order_weights(srw_handle *h, float p, float q, int32_t prev_id, const int32_t *prev_ids,
                                 int64_t n_prev, const int32_t *curr_ids, const float *curr_w, int64_t n,
                                 float *out_w);
/* RandomSample.secondOrderSample (:55-62) on the GPU. */
int32_t srw_second_order_sample(srw_handle *h, float p, float q, int32_t prev_id, const int32_t *prev_ids,
                                int64_t n_prev, const int32_t *curr_ids, const float *curr_w, int64_t n,
                                float r, int64_t *index);
/* The walk RNG stream evaluated on the GPU: out[i] = u(seed, iter[i], src[i], step[i]). */
int32_t srw_rng_uniform(srw_handle *h, uint32_t seed, const uint32_t *iter, const uint32_t *src,
                        const uint32_t *step, int64_t n, float *out);
/* The first-order pick through the 16-byte compact records (csrc/sampling.h:cfo_pick, what a p = q = 1 Philox walk does at every step)
 * on the row of `vertex`, one draw per element: m[i] < 2^24 is the lattice draw (p = m[i] * 2^-24), pos[i] the picked position inside
 * the row — RandomSample.sample's index for that p — and reads[i] the 16-byte records the pick loaded (1 where the guide entry's own
 * record is the answer).  Builds the compact table if the handle has none yet.  SRW_ERR_INVALID: no graph, a sharded handle, a
 * vertex that is absent / without neighbours / irregular (a negative or NaN weight), a draw >= 2^24, a graph whose compact table had
 * to be abandoned (a neighbour row too long for a link).  No reference counterpart: the reference scans the row. */
int32_t srw_cfo_pick(srw_handle *h, int32_t vertex, const uint32_t *m, int64_t n, int32_t *pos, int32_t *reads);

/* ---- host-only helpers (no GPU needed) ------------------------------------------------------ */
/* The edge-list tokenizer on its own: parses `path` into caller-visible arrays owned by the library
 * (released by srw_free).  Used by the CLI and by tests of the parse rules. */
int32_t srw_parse_edgelist(const char *path, int32_t weighted, int32_t partitioned, int32_t **src,
                           int32_t **dst, float **w, int32_t **pid, int64_t *n_lines, char *err, size_t errlen);
/* The --sources file of the CLI: vertex ids separated by white space / line ends, each token read by the rule of an edge
 * list's id column (Integer.parseInt, Unicode decimal digits included).  *ids (released by srw_free) holds *n ids in file
 * order; an empty file gives n = 0.  SRW_ERR_PARSE for a token that is no int32 ("line N: NumberFormatException ..."),
 * SRW_ERR_IO for a missing file ("Input path does not exist: ..."); the message goes to err. */
int32_t srw_parse_sources(const char *path, int32_t **ids, int64_t *n, char *err, size_t errlen);
void srw_free(void *p);
/* RandomWalk.save on host-resident paths (M/algorithm/RandomWalk.scala:234-241): same files as
 * srw_write_paths, for callers that assembled several walk calls themselves. */
int32_t srw_save_paths(const int32_t *paths, const int32_t *lens, int64_t n_walkers, int64_t stride,
                       const char *output_dir, int32_t n_parts, int32_t write_crc);
/* The chunk geometry of the per-edge bias table of a pair (prev -> curr) — what the planner, the table builder and the walk kernels
 * all compute from (deg(curr), deg(prev)) and the 10 policy words {min_shift, max_chunks, mask_max_deg, mask_min_prev_deg,
 * fine_min_prev_deg, fine_shift, fine_max_chunks, f32, u16, mask_ratio} (csrc/sampling.h:eb_pair_geometry).  Chunks of
 * 2^*chunk_shift candidates, *n_chunks of them, *masked = the pair carries chunk masks.  No reference counterpart (the reference
 * recomputes the biased weights of N(curr) at every step, RandomSample.scala:27-44); exported for the CPU test of the closed form. */
int32_t srw_table_geometry(int32_t deg_curr, int32_t deg_prev, const int32_t *policy, int32_t *chunk_shift, int32_t *n_chunks,
                           int32_t *masked);
/* Library / build identification ("stellar_rw gfx950 <git describe>"). */
const char *srw_version(void);

#ifdef __cplusplus
}
#endif
#endif
