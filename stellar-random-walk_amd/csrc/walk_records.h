// walk_records.h — records, argument blocks and host entry points shared by the walk kernels' translation units.
#pragma once
#include "engine.h"
#include "sampling.h"

namespace srw {

// Records shared by the whole-graph kernels and the vertex-sharded ones (described with the k_sh_* kernels in shard_kernels.hip).
struct alignas(16) WWalker { int32_t lw, src, prev, curr; };      // on the wire: 16 bytes
struct alignas(16) SWalker { int32_t lw, src, prev, curr, v, kind, pad0, pad1; };   // pad0: position of the chosen candidate (chain kernels)
enum : int32_t { SK_WALKER_RET = 1, SK_RET = 2, SK_DEAD = 3 };   // walker + return; return only (last step); death notice only
constexpr int CHAIN_CAP = 4096;     // draws on a CDF boundary per super-step / per launch that the chain kernels take (more: the general step)
struct alignas(16) ChainRec { uint32_t ri, pad; double S; };      // record index, (whole-graph walks: the step), the reference's sum of the biased row
// Whole-graph walks: where the table kernels leave a table step whose draw sits on a CDF boundary — one wire record per tie (lw = the
// iteration's offset) behind a chunk header, so that the chain kernels of the sharded walk read them like a super-step's input;
// k_walk_general, which redoes the handed-over walkers, takes the resolved step from the chain kernels' output.
struct TieSink {
  uint32_t *hdr;                  // [0] records written (the chunk header the chain kernels read)
  WWalker *recs;                  // [CHAIN_CAP]
  ChainRec *list;                 // [CHAIN_CAP]
  unsigned long long *cur;        // [2] ties met
  int32_t *todo_tie;              // per todo entry: its record, or -1
};

constexpr int TPB = 256;

// Waves per SIMD of the lean table kernels.  Round 2 (the exact chain still inlined): 4 waves/SIMD 221 M steps/s at config 3, 5
// 239 M, 6 235 M.  Round 3, with the chain out of these kernels (s25): config 3 (edge hash: request-bound) 5 -> 478 M, 6 -> 520 M,
// 7 -> 433 M; config 5's stand-in (row filters, no hash: latency-bound) 5 -> 290 M, 6 -> 326 M, 7 -> 348 M.  With one candidate per
// lane and round of the located chunk (SRW_RESOLVE_PER_LANE 1: fewer registers) and chunks of 64 (s59, A / B / C twice on one box):
// config 3 6 -> 705-719 M, 7 -> 771 M, 8 -> 690 M; config 5's stand-in 7 -> 363 M, 8 -> 387 M.  So by instantiation:
// Round 4, after the arguments left the SGPRs (TabArgs below: 65 VGPRs, no scratch at 7 waves; 64 VGPRs + 12 B at 8) and with SALU the
// busier unit (448 scalar against 302 vector instructions per step, profiles/r04_valu_issue.md): 8 waves 624 ms against 644 at config 3,
// 3 711 against 4 035 ms at config 5's stand-in (profiles/r04_table_kernel_ab_runs.txt, A / B / C twice on one box).
#ifndef SRW_LEAN_WAVES
#define SRW_LEAN_WAVES 8
#endif
// Round 4 (tree tables, 16-bit level 0, 4-byte ids; s125, one box): the row-filter instantiation at 8 waves/SIMD (64 VGPRs, 200 B of scratch
// per lane: 1.5 KB of spill writes per step reach the memory side at config 5's stand-in) 4 734 ms, 7 waves (72 VGPRs, 168 B) 4 637 ms, 6 waves 4 924 ms.
#ifndef SRW_LEAN_WAVES_BF
#define SRW_LEAN_WAVES_BF 8
#endif

// The table kernels take their arguments as ONE struct and read them again from the kernarg segment where a walker / a step
// needs them (device_common.h:fresh_args) instead of holding their ~130 dwords in SGPRs next to the walker's state.
struct TabArgs {
  GraphView g;                     // (first: fresh_graph() reads the same bytes)
  const int32_t *verts; int64_t n_verts, n_walkers; int32_t L, first_walk; RngSpec rng; float p, q;
  int32_t *paths, *lens; DevCounters *ctr; unsigned long long *cursor; int32_t *todo; unsigned long long *todo_n; TieSink tie;
};

// walk_lanes.hip: the table walk with one walker per lane; mode bit 0: mask rows per lane, bit 1: table steps per lane (0: every step served by the wave)
void launch_walk_tables_lanes(const TabArgs &ta, bool row_filters, int mode, int max_csh, int n_cus, hipStream_t st);

// The vertex-sharded walk's chunks (shard_kernels.hip); the chain kernels read a whole-graph walk's tie records through the same view.
constexpr int SHARD_MAX_WORLD = 64;
struct alignas(8) WRet { int32_t lw, v; };                         // on the wire: 8 bytes; lw top bit: death notice
// a record between the sampling kernel and the bucketing kernel (scratch, never on the wire): the forwarded walker
// (prev, curr), the vertex that goes home (v) and what to emit (kind)
constexpr int64_t SW_BYTES = 16, PR_BYTES = 8;
struct ShardIO {
  const char *recv;        // world chunks, one per sender
  int64_t chunk_bytes;
  int32_t cap_w, cap_r, world, rank, batch;
  // this rank's path staging (slot-major) and lengths: a return whose home is THIS rank is applied where it is produced
  // (no record): all of them at super-step 1 (every walker starts at home: n_local returns into one chunk otherwise —
  // world times the capacity an even spread needs), 1 / world of them later, every one at world 1
  int32_t *pt, *lens;
  int64_t n_rows;
};
struct ShardDst { char *p[SHARD_MAX_WORLD]; };   // where chunk (me -> d) is written

// chain_kernels.hip: the exact chain for the steps whose draw sits on a CDF boundary
struct alignas(16) ChainMeta { long long d_off; int32_t deg; uint32_t u_off; };   // first quotient in the scratch array, row length, first work unit
struct ChainUnits { double *usum; int32_t *ue; unsigned long long *utot; };       // per unit of 256 quotients: plain sum, guessed binade, integer increment
// Chain scratch of a handle: record list + meta + totals in one buffer, the quotients of up to d_cap candidates in another,
// the per-unit summaries in a third; behind them the whole-graph walk's tie records (TieSink), their output and a cursor of their own.
struct ChainBufs {
  ChainRec *list; ChainMeta *meta; uint32_t *totals; double *D; ChainUnits cu; long long d_cap;
  uint32_t *tie_hdr; WWalker *tie_recs; SWalker *tie_out; unsigned long long *tie_cur; uint32_t *tie_skip;
};
ChainBufs chain_bufs(srw_handle *h);
void enqueue_chain(srw_handle *h, const ChainBufs &cb, const GraphView &gv, const ShardIO &io, const srw_walk_params &P, int32_t step, int32_t last,
                   const RngSpec &rng, SWalker *scratch, int strat, unsigned long long *cursor, uint32_t *skipped, unsigned long long *pass_cur = nullptr);

// walk_kernels.hip: what the sharded walk's host side shares with the whole-graph one
void read_counters(srw_handle *h, srw_walk_stats *stats);
void check_params(const srw_walk_params &P);
// compacted ids (graph_build.hip:compact_ids): the kernels walked over ranks; the paths leave with the ids of the input
void paths_to_ids(srw_handle *h, int32_t *d_paths, const int32_t *d_lens, int64_t n_walkers, int64_t stride);

}  // namespace srw
