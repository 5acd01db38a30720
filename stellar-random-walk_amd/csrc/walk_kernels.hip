// walk_kernels.hip — the walk itself (gfx950).  Replaces RandomWalk.initFirstStep + the super-step loop of
// RandomWalk.randomWalk (M/algorithm/RandomWalk.scala:51-66, 95-139).
//
//   k_walk_first_order   p == q == 1: one walker per LANE, all walk_length+1 steps in one launch, O(1)
//                        exact sampling through the CDF+guide records (16 B, one sector per probe), paths
//                        staged in LDS and flushed as 64-byte runs.  HBM-latency/sector bound gather.
//   k_walk_general       any p, q: one walker per WAVE, persistent waves taking walkers from a counter; per step the
//                        first sampler that applies (sampling.h): search over exact prefix sums (specials binned by
//                        position in LDS, sorted-row intersection by probes / edge hash / id-window bitmap),
//                        certified parallel scan of the streamed row, or the reference's sequential f64 chain.
//   k_walk_alias         Mode A: per-vertex alias tables + rejection, one walker per lane.
//   k_walk_tables        q != 1 with a per-edge table for every pair: the lean table step, one walker per wave (walk_lanes.hip: per lane).
//   k_walk_q1            p != 1, q == 1: one walker per lane over the first-order guide table + exact prefix sums.
// The vertex-sharded multi-GPU path is shard_kernels.hip; the chain kernels that resolve boundary draws are chain_kernels.hip.
// No MFMA anywhere: integer/byte gather work bounded by HBM.
#include <algorithm>
#include <map>
#include <tuple>
#include <chrono>
#include <cstring>

#include "engine.h"
#include "sampling.h"
#include "walk_shared.h"

namespace srw {
namespace {
constexpr int TILE = 16;  // path slots staged in LDS between flushes (64 B per walker per flush)

// ---------------------------------------------------------------------------------------------------------
// How the LDS image (a ring of TILE slots per walker) goes out: a row is stored when the slot just written ends a 64-byte line of ITS
// addresses, so every run lies inside one aligned line (tests/path_flush_ref.py restates the rule).  LEGACY
// (SRW_WALK_LEGACY_FLUSH, the A/B arm of tools/first_order_ab.py --arm flush): every TILE steps, slots [s - 15, s] of every row — the runs
// start wherever the row does.  (128-byte lines over a ring of 32 slots, 32 KB per block: measured, 1.3 % against 1.7 % at RMAT-26,
// profiles/r08_path_flush.md.)
template <bool NT, int MINW, bool COMPACT, bool LEGACY>
__global__ __launch_bounds__(TPB, MINW) void k_walk_first_order(GraphView g, const int32_t *__restrict__ verts,
                                                          int64_t n_verts, int64_t n_walkers, int32_t L,
                                                          int32_t first_walk, RngSpec rng,
                                                          int32_t *__restrict__ paths, int32_t *__restrict__ lens,
                                                          DevCounters *ctr) {
  __shared__ int32_t tile[TPB / 64][64][TILE + 1];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int64_t wi = blockIdx.x * (int64_t)TPB + threadIdx.x;
  const int64_t wave_base = wi - lane;
  const int64_t stride = (int64_t)L + 2;
  bool alive = wi < n_walkers;
  uint32_t iter = 0; int32_t src = 0;
  Row r; r.off = 0; r.deg = 0; r.flags = 0;           // row descriptor of the current vertex
  if (alive) {
    int64_t it = wi / n_verts, vi = wi - it * n_verts;
    iter = (uint32_t)(first_walk + it);
    src = verts[vi];
    const Row *rp = row_of(g, src);
    if (rp) r = *rp;                                     // the only row-table access of the whole walk
  }
  int32_t len = 1;
  unsigned long long reads = 0, dead = 0, fb = 0;
  Bias nobias; nobias.second_order = false; nobias.need_member = false; nobias.p = nobias.q = 1.0f;
  nobias.prev = 0; nobias.prev_sids = nullptr; nobias.prev_deg = 0; nobias.vmin = g.vmin;
  tile[wv][lane][0] = src;
  // position of the row's slot 0 inside its 64-byte line, from the ADDRESS: any base pointer and any stride are right
  const uint32_t pbase = (uint32_t)(reinterpret_cast<uintptr_t>(paths) >> 2);
  const uint32_t a_own = (pbase + (uint32_t)wi * (uint32_t)stride) & (TILE - 1);
  if (!LEGACY && wi < n_walkers && a_own == TILE - 1) paths[wi * stride] = src;     // slot 0 ends a line: due at s = 0, a window of one slot
  src = rng_source(g, src);                            // from here on src only keys the Philox stream (compacted ids: the input's id)
  for (int32_t s = 1; s <= L + 1; ++s) {
    const int c = s & (TILE - 1);
    int32_t val = -1;
    if (alive) {
      if (r.deg == 0) {
        alive = false; if (s > 1) ++dead;                      // dead end, RandomWalk.scala:115-120 (acc2 counts the loop only)
      } else {
        if (COMPACT && !(r.flags & ROW_IRREGULAR)) {          // Philox draw on the 2^-24 lattice: 16-byte records
          const uint32_t m = walk_bits24(rng.seed, iter, (uint32_t)src, (uint32_t)s);
          unsigned rd;
          const CfoEnt e = cfo_pick<NT>(g.cfo + r.off, r.deg, m, rd, g.cfo_reload != 0); reads += rd;
          val = e.id; ++len;
          r.off = (int64_t)(e.link & CFO_NOFF_MASK); r.deg = (int32_t)((e.link >> 40) & 0x7FFFFFu);
          r.flags = (e.link >> 63) ? ROW_IRREGULAR : 0u;
        } else {
          float u = draw_uniform(rng, iter, (uint32_t)src, (uint32_t)s);
          FoEnt e;
          if (r.flags & ROW_IRREGULAR) {
            int32_t k = lane_pick_sequential(g.ent + r.off, r.deg, nobias, u);
            ++fb;
            if (COMPACT) {                                   // only the compact table exists: its links are valid for every row
              const CfoEnt ce = g.cfo[r.off + k];
              e.id = ce.id; e.noff = (int64_t)(ce.link & CFO_NOFF_MASK); e.ndeg = (int32_t)((ce.link >> 40) & 0x7FFFFFu);
              e.nflags = (ce.link >> 63) ? ROW_IRREGULAR : 0u;
            } else {
              e = g.fo[r.off + k];
            }
          } else {
            unsigned rd; int32_t k;
            e = fo_pick<NT>(g.fo + r.off, r.deg, u, k, rd); reads += rd;
          }
          val = e.id; ++len;
          r.off = e.noff; r.deg = e.ndeg; r.flags = e.nflags;   // the picked record carries the next row
        }
      }
    }
    tile[wv][lane][c] = val;
    if constexpr (LEGACY) {
      if (c == TILE - 1 || s == L + 1) {
        const int ncols = c + 1;
        const int64_t base_slot = s - c;
        __syncthreads();   // (the tile is private to the wave; a wave-level barrier measured the same, 64.1 vs 64.4 ms)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          int row = rr * 4 + (lane >> 4), col = lane & 15;
          int64_t w = wave_base + row;
          if (col < ncols && w < n_walkers) paths[w * stride + base_slot + col] = tile[wv][row][col];
        }
        __syncthreads();
      }
    } else {
      // due: slot s ends a line of this row, or the row.  A slot's ring entry is written again TILE steps later, after the row was due.
      const bool due = wi < n_walkers && ((((a_own + (uint32_t)s) & (TILE - 1)) == TILE - 1) || s == L + 1);
      unsigned long long todo = __ballot(due);
      if (todo) {                                        // (wave-uniform; the tile is private to the wave: LDS serves it in order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int grp = lane / TILE, col = lane & (TILE - 1);
        do {                                             // 64 / TILE due rows per store instruction, TILE lanes each
          int row = -1;
#pragma unroll
          for (int k = 0; k < 64 / TILE; ++k) {
            const int b = todo ? (int)__builtin_ctzll(todo) : -1;
            todo &= todo - 1;                            // (0 stays 0)
            if (grp == k) row = b;
          }
          if (row >= 0) {
            const int64_t w = wave_base + row;           // < n_walkers: the row was due
            const uint32_t a = (pbase + (uint32_t)w * (uint32_t)stride) & (TILE - 1);
            const int32_t t = s - (int32_t)((a + (uint32_t)s) & (TILE - 1)) + col;      // the line's first slot + col
            if (t >= 0 && t <= s) paths[w * stride + t] = tile[wv][row][t & (TILE - 1)];
          }
        } while (todo);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  if (wi < n_walkers) lens[wi] = len;
  flush_counters(ctr, (unsigned long long)(len - 1), dead, 0, 0, reads, fb);
}

__global__ __launch_bounds__(TPB, 4) void k_walk_general(GraphView g, const int32_t *__restrict__ verts,
                                                      int64_t n_verts, int64_t n_walkers, int32_t L,
                                                      int32_t first_walk, RngSpec rng, float p, float q,
                                                      int32_t *__restrict__ paths, int32_t *__restrict__ lens,
                                                      DevCounters *ctr, unsigned long long *cursor, int32_t tune,
                                                      const int32_t *__restrict__ todo, const unsigned long long *todo_n,
                                                      const int32_t *__restrict__ todo_tie, const ChainRec *__restrict__ tie_list,
                                                      const SWalker *__restrict__ tie_out) {
  __shared__ __attribute__((aligned(16))) uint32_t bitmap[TPB / 64][BINNED_LDS_WORDS];
  const int lane = lane_id();
  Member mem; mem.mode = 0; mem.bm = bitmap[threadIdx.x >> 6]; mem.seg_base = 0;
  mem.ehash = g.ehash; mem.ehash_mask = g.ehash_mask;
#ifdef SRW_PHASE_TIMING
  const unsigned long long t_begin = wall_clock64();
#endif
  const int64_t stride = (int64_t)L + 2;
  unsigned long long steps = 0, degc = 0, degp = 0, fb = 0, dead = 0, fast = 0, srch = 0;
  unsigned long long n_strat[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // SRW_STRAT_*
  // Persistent waves: a walker costs anything from a few to millions of entry reads, and a block's LDS is only
  // released when its slowest wave ends — so every wave takes the next walker from a counter instead of owning one.
  while (true) {
    unsigned long long grab = 0;
    if (lane == 0) grab = atomicAdd(cursor, 1ull);
    int64_t wi = (int64_t)(((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(grab >> 32)) << 32) |
                           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)grab));
    int32_t tie_s = -1, tie_k = 0, tie_next = 0;     // the walker's step the chain kernels resolved (k_walk_tables' tie), if any
    if (todo) {                                      // only the walkers k_walk_tables handed over
      if (wi >= (int64_t)*todo_n) break;
      if (todo_tie) {
        const int32_t ci = todo_tie[wi];
        if (ci >= 0) {
          const SWalker o = tie_out[ci];
          if (o.kind == SK_WALKER_RET || o.kind == SK_RET) { tie_s = (int32_t)tie_list[ci].pad; tie_k = o.pad0; tie_next = o.curr; }
        }
      }
      wi = todo[wi];
    } else if (wi >= n_walkers) break;
    int64_t it = wi / n_verts, vi = wi - it * n_verts;
    const uint32_t iter = (uint32_t)(first_walk + it);
    const int32_t src = verts[vi];
    const uint32_t ksrc = (uint32_t)rng_source(g, src);   // Philox key: the input's id of the source
    int32_t *path = paths + wi * stride;
    if (lane == 0) path[0] = src;
    int32_t prev = src, curr = src, len = 1;
    Row rprev; rprev.off = 0; rprev.deg = 0; rprev.flags = 0;
    int64_t eprev = 0;                               // entry index of the edge (prev -> curr) the walker arrived by
    for (int32_t s = 1; s <= L + 1; ++s) {
      // the step's first round trip: the row of curr and the (prev -> curr) pair's table word, issued together
      const bool second = s > 1;
      const int64_t cslot = (int64_t)curr - g.vmin;
      const bool in_range = cslot >= 0 && cslot < g.n_slots;
      const bool want_tab = g.eb_off && second && q != 1.0f && !(tune & 16);
      Row r = g.rows[in_range ? cslot : 0];
      uint32_t eo = EB_NONE;
      if (want_tab) eo = g.eb_off[eprev];
      if (!in_range) { r.off = 0; r.deg = 0; r.flags = 0; }
      if (r.deg == 0) { dead += s > 1; break; }
      Bias b;                                          // N(prev) = last step's row (whole-graph handle)
      b.p = p; b.q = q; b.prev = prev; b.second_order = second; b.need_member = second && (q != 1.0f); b.vmin = g.vmin;
      b.prev_sids = g.sids + rprev.off; b.prev_deg = rprev.deg; b.prev_hub = rprev.flags >> ROW_HUB_SHIFT;
      float u = draw_uniform(rng, iter, ksrc, (uint32_t)s);
      unsigned f = 0, sv = 0;
#ifdef SRW_PHASE_TIMING
      mem.t_step0 = wall_clock64();
#endif
      SRW_T0(mem);
      int32_t k = -1, next = 0;
      bool binned_served = false, have_next = false;
      unsigned which = SRW_STRAT_SCAN;
      if (s == tie_s) { k = tie_k; next = tie_next; have_next = true; binned_served = true; which = SRW_STRAT_EDGE_TABLE; f = 1; n_strat[SRW_STAT_TIES_RESOLVED] += 1; }
      else if (want_tab) {
        if (r.deg <= g.eb_mask_max) {
          // membership mask of the pair (inline for rows up to 32 candidates): no lookup, the row sits in registers
          if (r.deg <= 32 || eo != EB_NONE) {
            k = wave_pick_masked(g, r, b, eo, r.deg > 32 ? g.em_bits + (size_t)eo * 4 : nullptr, u, f, next);
            have_next = true; binned_served = true; which = SRW_STRAT_EDGE_MASK;
            srch += 8ull * (unsigned long long)r.deg + 4ull * (unsigned long long)((r.deg + 31) >> 5);
          }
        } else if (eo != EB_NONE && (r.flags & ROW_PQ_OK)) {
          // chunk prefixes of the pair's corrections: search + one chunk, no intersection
          k = wave_pick_edge_table(g, r, b, g.eb_bins + (size_t)eo * 8, u, f, sv, mem, next, mem.bm + 2 * BIN_CAP);
          if (k >= 0) { have_next = true; binned_served = true; which = SRW_STRAT_EDGE_TABLE; srch += 8ull * EB_BINS; }
        }
      }
      // search over exact prefix sums: a short list of specials (return edges only) when q == 1, position bins else
      if (k < 0 && (!b.need_member || (tune & 16))) {
        k = wave_pick_prefix(g, r, cslot, b, mem.bm, u, f, sv);
        if (k >= 0) which = SRW_STRAT_PREFIX;
      }
      SRW_T1(mem, t_prefix);
      if (k < 0 && !(tune & 16)) {
        unsigned su = 0;
        k = wave_pick_binned(g, r, cslot, b, mem.bm, u, f, sv, tune & 7, (tune & 8) != 0, mem, srch, su, next);
        binned_served = k >= 0;                             // srch: bytes its membership strategy read (bench.py)
        if (k >= 0) { have_next = true; which = su == 1 ? SRW_STRAT_P1 : su == 2 ? SRW_STRAT_P2 : su == 4 ? SRW_STRAT_P3 : SRW_STRAT_W; }
      }
      if (k < 0) { k = wave_pick_scan(g, r, b, mem, u, f); degc += (unsigned long long)r.deg; }
      else { fast += sv; }
      n_strat[which] += 1; n_strat[SRW_STRAT_CHAIN] += f;
      if (!have_next) next = g.ent[r.off + k].id;
#ifdef SRW_PHASE_TIMING
      mem.t_strat[which] += wall_clock64() - mem.t_step0 + (unsigned long long)(next & 0);   // (next: the id load is part of the step)
#endif
      fb += f;
      if (b.need_member && !binned_served) degp += (unsigned long long)b.prev_deg;
      if (lane == 0) path[s] = next;
      prev = curr; curr = next; ++len; rprev = r; eprev = r.off + k;
    }
    for (int64_t t = len + lane; t < stride; t += 64) path[t] = -1;  // unused tail
    if (lane == 0) lens[wi] = len;
    steps += (unsigned long long)(len - 1);
  }
  if (lane == 0) {
    if (steps) atomicAdd(&ctr->steps, steps);
    if (dead) atomicAdd(&ctr->dead_ends, dead);
    if (degc) atomicAdd(&ctr->sum_deg_curr, degc);
    if (degp) atomicAdd(&ctr->sum_deg_prev, degp);
    if (fb) atomicAdd(&ctr->fallbacks, fb);
    if (fast) atomicAdd(&ctr->ent_reads, fast);      // general kernel: steps served by the prefix-sum search
    srch += mem.res_bytes;
    if (srch) atomicAdd(&ctr->trials, srch);         // ... and the bytes the binned ones' membership strategies read
    for (int i = 0; i < 12; ++i) if (n_strat[i]) atomicAdd(&ctr->strat[i], n_strat[i]);
#ifdef SRW_PHASE_TIMING
    const unsigned long long tv[10] = {wall_clock64() - t_begin, mem.t_prefix, mem.t_a, mem.t_p1, mem.t_p2, mem.t_w,
                                       mem.t_fin, mem.t_fill, mem.t_pass1, mem.t_pass2};
    for (int i = 0; i < 10; ++i) atomicAdd(&ctr->dbg[i], tv[i] >> 10);
    atomicAdd(&ctr->dbg[10], mem.n_w); atomicAdd(&ctr->dbg[11], mem.n_w_elems); atomicAdd(&ctr->dbg[12], mem.n_w_windows);
    atomicAdd(&ctr->dbg[13], mem.n_p1); atomicAdd(&ctr->dbg[14], mem.n_p1_elems); atomicAdd(&ctr->dbg[15], mem.n_binned);
    for (int i = 0; i < 12; ++i) atomicAdd(&ctr->dbg[24 + i], mem.t_strat[i] >> 10);
    atomicAdd(&ctr->dbg[16], mem.t_w_lb >> 10); atomicAdd(&ctr->dbg[17], mem.t_w_ins >> 10); atomicAdd(&ctr->dbg[18], mem.t_w_la >> 10); atomicAdd(&ctr->dbg[19], mem.t_w_probe >> 10);
#endif
  }
}

// ---------------------------------------------------------------------------------------------------------
// The same walk for the walkers whose EVERY step finds a per-edge table (edge_tables.hip): first step on the raw row,
// then membership masks / chunk-prefix tables only.  Without the on-the-fly samplers the kernel needs a fraction of
// k_walk_general's registers (128 VGPRs + scratch there) and 4 KB of LDS per wave, so more waves hide the dependent
// round trips of a step.  A walker that meets a pair without a table is handed over untouched (its index goes to
// `todo`; k_walk_general redoes it from its first step: the keyed RNG makes that the same path).
// The lean table kernel takes its arguments as ONE struct and reads them again from the kernarg segment where a walker / a step
// needs them (device_common.h:fresh_args) instead of holding their ~130 dwords in SGPRs next to the walker's state.
#define TAB_ARGS() fresh_args<TabArgs>()
#define GFRESH() fresh_graph()
template <bool BF>   // BF: the located chunk's probes of a long N(prev) go through the row filters (no edge hash; GraphView::bf_off)
__global__ __launch_bounds__(TPB, BF ? SRW_LEAN_WAVES_BF : SRW_LEAN_WAVES) void k_walk_tables(TabArgs a0) {
  __shared__ __attribute__((aligned(16))) uint32_t stage_all[TPB / 64][1024];
  const int lane = lane_id();
  uint32_t *stage = stage_all[threadIdx.x >> 6];
  Member mem; mem.mode = 0; mem.bm = stage; mem.seg_base = 0;
  const int32_t L = a0.L;
  const int64_t stride = (int64_t)L + 2;
  unsigned long long steps = 0, srch = 0;
  uint32_t fb = 0, dead = 0, fast = 0, n_tab = 0, n_mask = 0, n_first = 0;
  while (true) {
    unsigned long long grab = 0;
    const TabArgs aw = TAB_ARGS();                    // (what a walker's start needs)
    if (lane == 0) grab = atomicAdd(aw.cursor, 1ull);
    const int64_t wi = (int64_t)(((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(grab >> 32)) << 32) |
                                 (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)grab));
    if (wi >= aw.n_walkers) break;
    const int64_t it = wi / aw.n_verts, vi = wi - it * aw.n_verts;
    const uint32_t iter = (uint32_t)(aw.first_walk + it);
    const int32_t src = __builtin_amdgcn_readfirstlane(aw.verts[vi]);
    const uint32_t ksrc = (uint32_t)__builtin_amdgcn_readfirstlane(rng_source(aw.g, src));
    int32_t *path = aw.paths + wi * stride;
    if (lane == 0) path[0] = src;
    int32_t prev = src, curr = src, len = 1;
    Row rprev; rprev.off = 0; rprev.deg = 0; rprev.flags = 0;
    int64_t eprev = 0;
    uint32_t w_fb = 0, w_dead = 0, w_fast = 0, w_srch = 0, w_tab = 0, w_mask = 0;    // (a handed-over walker is not counted here)
    bool handed_over = false;
    int32_t tie_rec = -1;
    WaveDraws draws;
    for (int32_t s = 1; s <= L + 1; ++s) {
      const bool second = s > 1;
      const TabArgs as = TAB_ARGS();                  // (vmin, n_slots, rows, eb_off, the mask geometry, p, q, the seed: what the top of a step needs)
      const GraphView &gs = as.g;
      const int64_t cslot = (int64_t)curr - gs.vmin;
      const bool in_range = cslot >= 0 && cslot < gs.n_slots;
      Row r = gs.rows[in_range ? cslot : 0];
      uint32_t eo = EB_NONE;
      if (second) eo = gs.eb_off[eprev];
      r = uniform_row(r); eo = (uint32_t)__builtin_amdgcn_readfirstlane((int)eo);
      if (!in_range) { r.off = 0; r.deg = 0; r.flags = 0; }
      if (r.deg == 0) { w_dead += s > 1; break; }
      const float u = draws.at(as.rng, iter, ksrc, s, 1);
      unsigned f = 0, sv = 0;
      int32_t k, next = 0;
      // (CHAIN = false: the exact chain is not in this kernel — a draw within rounding distance of a CDF boundary hands the
      //  walker over like a missing table; the chain's registers and scratch cost every step otherwise)
      if (!second) {
        k = uni(wave_pick_first<false>(GFRESH(), r, u, f, next));       // (uni: the pick is the wave's — a loop exit the compiler can see is uniform keeps the walker's state scalar)
        if (k < 0) { handed_over = true; break; }
      } else {
        Bias b;
        b.p = as.p; b.q = as.q; b.prev = prev; b.second_order = true; b.need_member = true; b.vmin = gs.vmin;
        b.prev_sids = gs.sids + rprev.off; b.prev_deg = rprev.deg; b.prev_hub = rprev.flags >> ROW_HUB_SHIFT;
        SRW_T0(mem);
        if (r.deg <= gs.eb_mask_max && (r.deg <= 32 || eo != EB_NONE)) {
          k = uni(wave_pick_masked<false>(GFRESH(), r, b, eo, r.deg > 32 ? gs.em_bits + (size_t)eo * 4 : nullptr, u, f, next));
          w_mask += 1; w_srch += 8u * (uint32_t)r.deg + 4u * (uint32_t)((r.deg + 31) >> 5);
          SRW_T1(mem, t_a);
        } else if (r.deg > gs.eb_mask_max && eo != EB_NONE && (r.flags & ROW_PQ_OK)) {
          double S_tie = 0.0;
          k = uni(wave_pick_edge_table<BF, false>(GFRESH(), r, b, gs.eb_bins + (size_t)eo * 8, u, f, sv, mem, next, stage, &S_tie));
          if (k >= 0) { w_tab += 1; w_srch += 8u * EB_BINS; w_fast += sv; }
          else if (k == CHAIN_NEEDED && as.tie.list) {   // a tie on a table step: its exact chain by the chain kernels (the whole GPU)
            const TieSink tie = TAB_ARGS().tie;
            if (lane == 0) {
              const unsigned long long c = atomicAdd(tie.cur, 1ull);
              if (c < (unsigned long long)CHAIN_CAP) {
                tie_rec = (int32_t)c;
                WWalker wr; wr.lw = (int32_t)it; wr.src = src; wr.prev = prev; wr.curr = curr; tie.recs[c] = wr;
                ChainRec cr; cr.ri = (uint32_t)c; cr.pad = (uint32_t)s; cr.S = S_tie; tie.list[c] = cr;
                atomicAdd(tie.hdr, 1u);
              }
            }
          }
          SRW_T1(mem, t_p1);
#ifdef SRW_PHASE_TIMING
          if (rprev.deg > 1024) mem.t_p2 += wall_clock64() - mem.t_mark;      // ... of which steps with a long N(prev)
#endif
        } else k = -1;
        k = uni(k);                                        // (after the lane-0 region above: its join would make the pick look divergent)
        if (k < 0) { handed_over = true; break; }          // no table for this pair: the general kernel takes the walker
      }
      next = uni(next);
      w_fb += f;
      if (lane == 0) path[s] = next;
      prev = curr; curr = next; ++len; rprev = r; eprev = r.off + k;
    }
    if (handed_over) {
      const TabArgs ah = TAB_ARGS();
      if (lane == 0) {
        const unsigned long long t = atomicAdd(ah.todo_n, 1ull);
        ah.todo[t] = (int32_t)wi;
        if (ah.tie.todo_tie) ah.tie.todo_tie[t] = tie_rec;
        atomicAdd(&ah.ctr->strat[SRW_STAT_HANDED_OVER], 1ull);
      }
      continue;
    }
    for (int64_t t = len + lane; t < stride; t += 64) path[t] = -1;  // unused tail
    if (lane == 0) TAB_ARGS().lens[wi] = len;
    steps += (unsigned long long)(len - 1); n_first += len > 1 ? 1u : 0u;
    fb += w_fb; dead += w_dead; fast += w_fast; srch += w_srch; n_tab += w_tab; n_mask += w_mask;
  }
  if (lane == 0) {
    DevCounters *ctr = TAB_ARGS().ctr;
    srch += mem.res_bytes;
    if (steps) atomicAdd(&ctr->steps, steps);
    if (dead) atomicAdd(&ctr->dead_ends, (unsigned long long)dead);
    if (fb) { atomicAdd(&ctr->fallbacks, (unsigned long long)fb); atomicAdd(&ctr->strat[SRW_STRAT_CHAIN], (unsigned long long)fb); }
    if (fast) atomicAdd(&ctr->ent_reads, (unsigned long long)fast);
    if (srch) atomicAdd(&ctr->trials, srch);
    if (n_tab) atomicAdd(&ctr->strat[SRW_STRAT_EDGE_TABLE], (unsigned long long)n_tab);
    if (n_mask) atomicAdd(&ctr->strat[SRW_STRAT_EDGE_MASK], (unsigned long long)n_mask);
    if (n_first) atomicAdd(&ctr->strat[SRW_STRAT_SCAN], (unsigned long long)n_first);
#ifdef SRW_PHASE_TIMING
    // lean kernel: dbg[1] mask-step time, [2] table-step time, [3] ... with deg(prev) > 1024, [10..15] resolve statistics
    atomicAdd(&ctr->dbg[1], mem.t_a >> 10); atomicAdd(&ctr->dbg[2], mem.t_p1 >> 10); atomicAdd(&ctr->dbg[3], mem.t_p2 >> 10);
    atomicAdd(&ctr->dbg[10], mem.n_w); atomicAdd(&ctr->dbg[11], mem.n_w_elems); atomicAdd(&ctr->dbg[12], mem.n_w_windows);
    atomicAdd(&ctr->dbg[13], mem.n_p1); atomicAdd(&ctr->dbg[14], mem.n_p1_elems); atomicAdd(&ctr->dbg[15], mem.n_binned);
    atomicAdd(&ctr->dbg[16], mem.t_fin);
#endif
  }
}

// p != 1, q == 1: the only biased candidates are the return edges, so a step is a first-order step plus one
// correction — one walker per LANE, like k_walk_first_order (r01 ran this case one walker per wave: 4.6e8 steps/s).
// Per step, under the row certificate of sampler_tables.hip (every prefix sum exact):
//   A'_k = PQ[k] + sum over the return edges r_i <= k of c_i,  r_i from rev[e] (multi-edges: four in registers, more by loop), c_i = fl(w_i / p) - w_i,
//   S = PQ[deg-1] + sum of all c_i
// and the reference's acc_k = sum of fl(w'_i / S) differs from A'_k / S by at most (k + 2) u A'_k / S — the certified
// divide-free compares of binned_resolve.  The first k that is not a certain miss is located from the first-order guide
// table (a start position; the exact prefix sums decide; a saturated guide entry or a start more than a few positions
// off — rows with many parallel return edges — is replaced by a bisection) and must be a certain hit, else the walker is
// handed over to k_walk_general, as are walkers that meet an irregular row.
// The picked compact record carries the next row descriptor, as in k_walk_first_order.
template <bool NT>
__global__ __launch_bounds__(TPB) void k_walk_q1(GraphView g, const int32_t *__restrict__ verts, int64_t n_verts,
                                                 int64_t n_walkers, int32_t L, int32_t first_walk, RngSpec rng, float p,
                                                 int32_t *__restrict__ paths, int32_t *__restrict__ lens, DevCounters *ctr,
                                                 int32_t *__restrict__ todo, unsigned long long *todo_n, uint32_t max_ret) {
  __shared__ int32_t tile[TPB / 64][64][TILE + 1];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int64_t wi = blockIdx.x * (int64_t)TPB + threadIdx.x;
  const int64_t wave_base = wi - lane;
  const int64_t stride = (int64_t)L + 2;
  bool alive = wi < n_walkers, handed = false;
  uint32_t iter = 0; int32_t src = 0;
  Row r; r.off = 0; r.deg = 0; r.flags = 0;
  if (alive) {
    const int64_t it = wi / n_verts, vi = wi - it * n_verts;
    iter = (uint32_t)(first_walk + it);
    src = verts[vi];
    const Row *rp = row_of(g, src);
    if (rp) r = *rp;
  }
  int32_t len = 1;
  int64_t eprev = 0;
  int32_t prev_id = src, curr_id = src;
  unsigned long long reads = 0, dead = 0;
  tile[wv][lane][0] = src;
  src = rng_source(g, src);                            // from here on src only keys the Philox stream
  for (int32_t s = 1; s <= L + 1; ++s) {
    const int c = s & (TILE - 1);
    int32_t val = -1;
    bool big = false; uint32_t big_rv = 0u, big_m = 0u;
    if (alive) {
      if (r.deg == 0) {
        alive = false; if (s > 1) ++dead;
      } else if (r.flags & ROW_IRREGULAR) {
        alive = false; handed = true; atomicAdd(&ctr->why[0], 1ull);
      } else {
        const uint32_t m = walk_bits24(rng.seed, iter, (uint32_t)src, (uint32_t)s);
        const CfoEnt *crow = g.cfo + r.off;
        CfoEnt e; int32_t k = -1;
        if (s == 1) {                               // initFirstStep: raw weights = the first-order draw
          unsigned rd; e = cfo_pick<NT>(crow, r.deg, m, rd, k, g.cfo_reload != 0); reads += rd;
        } else {
          const int4v rv4 = NT ? __builtin_nontemporal_load(reinterpret_cast<const int4v *>(g.rev + eprev))
                               : *reinterpret_cast<const int4v *>(g.rev + eprev);
          if ((uint32_t)rv4.x != REV_NONE && ((uint32_t)rv4.x >> 24) > max_ret) { big = true; big_rv = (uint32_t)rv4.x; big_m = m; }
          else {
            const int why = q1_pick<NT>(g, r, crow, (uint32_t)rv4.x, rv4.y, __int_as_float(rv4.z), prev_id, m, p, e, k, reads);
            if (why) { alive = false; handed = true; atomicAdd(&ctr->why[why], 1ull); }
          }
        }
        if (alive && !big) {
          val = e.id; ++len;
          prev_id = curr_id; curr_id = val;
          eprev = r.off + k;
          r.off = (int64_t)(e.link & CFO_NOFF_MASK); r.deg = (int32_t)((e.link >> 40) & 0x7FFFFFu);
          r.flags = (e.link >> 63) ? ROW_IRREGULAR : 0u;
        }
      }
    }
    // Steps with many parallel return edges (a hub's self-loops, hub <-> hub multi-edges: up to hundreds): q1_pick walks the run once
    // per prefix value in ONE lane while 63 wait — the wave takes them one at a time instead (wave_pick_returns).
    unsigned long long mb = __ballot(big);
    while (mb) {
      const int l = __ffsll((long long)mb) - 1;
      mb &= mb - 1ull;
      Row rr;
      rr.off = (int64_t)(((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)r.off >> 32), l) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)r.off, l));
      rr.deg = __builtin_amdgcn_readlane(r.deg, l); rr.flags = ROW_PQ_OK;          // (q1 runs only when every row holds the certificate)
      const int32_t pv = __builtin_amdgcn_readlane(prev_id, l);
      const uint32_t rvl = (uint32_t)__builtin_amdgcn_readlane((int)big_rv, l);
      const uint32_t ml = (uint32_t)__builtin_amdgcn_readlane((int)big_m, l);
      const int64_t so = rr.off + (int64_t)(rvl & 0xFFFFFFu);
      int32_t nr = (int32_t)(rvl >> 24);
      if (nr >= 255) {                                     // the count saturated: the run of prev in the sorted row
        const uint32_t xprev = (uint32_t)((int64_t)pv - g.vmin);
        nr = 0;
        for (int64_t cc = so;; cc += 64) {
          const unsigned long long mm = __ballot(cc + lane < rr.off + rr.deg && g.sids[cc + lane] == xprev);
          nr += __popcll(mm);
          if (mm != ~0ull) break;
        }
      }
      Bias b; b.p = p; b.q = 1.0f; b.prev = pv; b.second_order = true; b.need_member = false; b.vmin = g.vmin;
      b.prev_sids = nullptr; b.prev_deg = 0; b.prev_hub = 0;
      unsigned f = 0;
      const int32_t kk = wave_pick_returns<false>(g, rr, b, so, nr, (float)ml * (1.0f / 16777216.0f), f);
      if (lane == l) {
        big = false;
        if (kk < 0) { alive = false; handed = true; atomicAdd(&ctr->why[kk == CHAIN_NEEDED ? 2 : 1], 1ull); }
        else {
          const CfoEnt e = load_cfo<NT>(g.cfo + r.off + kk); ++reads;
          val = e.id; ++len;
          prev_id = curr_id; curr_id = val;
          eprev = r.off + kk;
          r.off = (int64_t)(e.link & CFO_NOFF_MASK); r.deg = (int32_t)((e.link >> 40) & 0x7FFFFFu);
          r.flags = (e.link >> 63) ? ROW_IRREGULAR : 0u;
        }
      }
    }
    tile[wv][lane][c] = val;
    if (c == TILE - 1 || s == L + 1) {
      const int ncols = c + 1;
      const int64_t base_slot = s - c;
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        int row = rr * 4 + (lane >> 4), col = lane & 15;
        int64_t w = wave_base + row;
        if (col < ncols && w < n_walkers) paths[w * stride + base_slot + col] = tile[wv][row][col];
      }
      __syncthreads();
    }
  }
  if (wi < n_walkers) {
    if (handed) { todo[atomicAdd(todo_n, 1ull)] = (int32_t)wi; atomicAdd(&ctr->strat[SRW_STAT_HANDED_OVER], 1ull); }   // k_walk_general redoes it from its first step
    else lens[wi] = len;
  }
  const unsigned long long my_steps = handed ? 0ull : (unsigned long long)(len - 1);
  flush_counters(ctr, my_steps, handed ? 0ull : dead, 0, 0, reads, 0);
  const unsigned long long tot = wave_sum_u64(my_steps);
  if (lane == 0 && tot) atomicAdd(&ctr->strat[SRW_STRAT_Q1_LANE], tot);
}

// ---------------------------------------------------------------------------------------------------------
// Mode A: per-vertex alias draw + rejection for the p/q bias (KnightKing-style), one walker per lane, each lane
// its own (step, trial) state machine so that lanes do not wait for each other's rejections.  Spec shared with
// oracle/srw_oracle.c:alias_pick — trial t of step s draws Philox(ctr = (iter, src, s, t), key = (seed, 0xA11A5)):
// slot j = ((x0:x1) * deg) >> 64, coin u2 = (x2 >> 8) 2^-24 keeps j or takes alias[j]; a second-order step accepts
// iff u3 * Q < bias, u3 = (x3 >> 8) 2^-24, Q = max(1, 1/q), bias = 1/p | 1 | 1/q; when 1/p > Q the excess
// (1/p - Q) * w of the return edge(s) is sampled by an appendix branch chosen by area (KnightKing's outlier folding).
// A trial needs only the first 16 bytes of the record (prob, alias, id, reverse weight); the link to the next row is
// fetched when the trial is ACCEPTED (same 64-byte sector: an L2 hit) — rejected trials return half the bytes.
template <bool NT>
__device__ inline AEnt load_al_head(const AEnt *p) {
  const int4v *q = reinterpret_cast<const int4v *>(p);
  const int4v a = NT ? __builtin_nontemporal_load(q) : *q;
  AEnt e;
  e.prob = __int_as_float(a.x); e.alias = a.y; e.id = a.z; e.wrev = __int_as_float(a.w);
  e.noff = 0; e.ndeg = 0; e.nflags = 0;
  return e;
}
template <bool NT>
__device__ inline void load_al_tail(const AEnt *p, AEnt &e) {
  const int4v *q = reinterpret_cast<const int4v *>(p) + 1;
  const int4v b = NT ? __builtin_nontemporal_load(q) : *q;
  e.noff = (int64_t)(((uint64_t)(uint32_t)b.y << 32) | (uint32_t)b.x);
  e.ndeg = b.z; e.nflags = (uint32_t)b.w;
}

template <bool NT>
__global__ __launch_bounds__(TPB, 6) void k_walk_alias(GraphView g, const int32_t *__restrict__ verts, int64_t n_verts,
                                                    int64_t n_walkers, int32_t L, int32_t first_walk, uint32_t seed,
                                                    float p, float q, int32_t *__restrict__ paths,
                                                    int32_t *__restrict__ lens, DevCounters *ctr) {
  // Lanes reject independently, so they are not in step: each lane stages its own 16 path slots in LDS and writes
  // them as one 64-byte run (16 scattered 4-byte stores per run cost 16 L2-miss-path requests instead of 1).
  __shared__ int32_t stage[TPB][TILE + 1];
  int32_t *buf = stage[threadIdx.x];
  const int64_t wi = blockIdx.x * (int64_t)TPB + threadIdx.x;
  unsigned long long reads = 0, dead = 0, fb = 0, trials = 0;
  int32_t len = 0;
  if (wi < n_walkers) {
    const int64_t stride = (int64_t)L + 2;
    const int64_t it = wi / n_verts, vi = wi - it * n_verts;
    const uint32_t iter = (uint32_t)(first_walk + it);
    const int32_t src = verts[vi];
    const uint32_t ksrc = (uint32_t)rng_source(g, src);   // Philox key: the input's id of the source
    int32_t *path = paths + wi * stride;
    Row rc; rc.off = 0; rc.deg = 0; rc.flags = 0;
    { const Row *rp0 = row_of(g, src); if (rp0) rc = *rp0; }
    Row rp = rc;
    int32_t curr = src, prev = src;
    buf[0] = src; len = 1;
    const float inv_p = 1.0f / p, inv_q = 1.0f / q;
    const float Q = inv_q > 1.0f ? inv_q : 1.0f;                  // envelope WITHOUT the return edge
    const bool biased_cfg = !(p == 1.0f && q == 1.0f);
    int32_t s = 1; uint32_t t = 0;
    // outlier folding state of the current step (valid while t > 0)
    bool fold = false; double fa = 0.0, ftot = 0.0, fw = 0.0; int32_t flo = -1, fhi = -1;
    float wprev_hint = __int_as_float(0x7FC00000);   // W_prev carried by the record that led here (NaN: unknown)
    while (s <= L + 1) {
      if (rc.deg == 0) { if (s > 1) ++dead; break; }
      const bool second = s > 1, biased = second && biased_cfg;
      uint32_t o[4];
      philox4x32_10(iter, ksrc, (uint32_t)s, t, seed, 0xA11A5u, o);
      AEnt e;
      const AEnt *ep = nullptr;                 // record whose link is still to be fetched
      bool accepted = true;
      if (rc.flags & ROW_ALIAS_IRREGULAR) {     // not alias-regular: the reference's CDF inversion, literally
        Bias b; b.p = p; b.q = q; b.prev = prev; b.second_order = second; b.need_member = second && q != 1.0f;
        b.prev_sids = g.sids + rp.off; b.prev_deg = rp.deg; b.vmin = g.vmin;
        float u = (float)(o[2] >> 8) * (1.0f / 16777216.0f);
        int32_t k = lane_pick_sequential(g.ent + rc.off, rc.deg, b, u);
        e = g.al[rc.off + k]; ++fb;
      } else {
        if (t == 0) {            // once per step: does the return edge stick out of the envelope?
          fold = false;
          if (biased && inv_p > Q) {
            flo = -1; fhi = -1;
            if (wprev_hint == wprev_hint) {
              fw = (double)wprev_hint;          // exact: precomputed at build time with the same f64 sum
            } else {
              // occurrences of prev in N(curr): equal range in the sorted row; weights in input order via sperm
              const uint32_t *cs = g.sids + rc.off;
              const uint32_t x = (uint32_t)((int64_t)prev - g.vmin);
              int32_t lo = 0, hi = rc.deg;
              while (lo < hi) { int32_t mid = lo + ((hi - lo) >> 1); if (cs[mid] < x) lo = mid + 1; else hi = mid; }
              flo = lo; fhi = lo; fw = 0.0;
              while (fhi < rc.deg && cs[fhi] == x) { fw += (double)g.ent[rc.off + g.sperm[rc.off + fhi]].w; ++fhi; }
            }
            if (fw > 0.0) {
              const double S = g.rsum[(int64_t)curr - g.vmin];
              fa = ((double)inv_p - (double)Q) * fw; ftot = (double)Q * S + fa; fold = true;
            }
          }
        }
        bool appendix = false;
        if (fold) {
          uint32_t y[4];
          philox4x32_10(iter, ksrc, (uint32_t)s, t, seed, 0xA11A6u, y);
          const float u5 = (float)(y[0] >> 8) * (1.0f / 16777216.0f);
          if ((double)u5 * ftot < fa) {       // appendix: return to prev; occurrence ~ w in input order
            appendix = true;
            if (flo < 0) {                      // the occurrences were not needed until now: find them
              const uint32_t *cs = g.sids + rc.off;
              const uint32_t x = (uint32_t)((int64_t)prev - g.vmin);
              int32_t lo = 0, hi = rc.deg;
              while (lo < hi) { int32_t mid = lo + ((hi - lo) >> 1); if (cs[mid] < x) lo = mid + 1; else hi = mid; }
              flo = lo; fhi = lo;
              while (fhi < rc.deg && cs[fhi] == x) ++fhi;
            }
            const float u6 = (float)(y[1] >> 8) * (1.0f / 16777216.0f);
            const double target = (double)u6 * fw;
            double cum = 0.0; int32_t pos = g.sperm[rc.off + flo];
            for (int32_t c = flo; c < fhi; ++c) {
              pos = (int32_t)g.sperm[rc.off + c];
              cum += (double)g.ent[rc.off + pos].w;
              if (cum >= target) break;
            }
            ep = g.al + rc.off + pos; e = load_al_head<NT>(ep); ++reads;
          }
        }
        ++trials;
        if (!appendix) {
          const uint64_t r64 = ((uint64_t)o[0] << 32) | o[1];
          const int64_t j = (int64_t)__umul64hi(r64, (uint64_t)(uint32_t)rc.deg);
          ep = g.al + rc.off + j; e = load_al_head<NT>(ep); ++reads;
          const float u2 = (float)(o[2] >> 8) * (1.0f / 16777216.0f);
          if (!(u2 < e.prob)) { ep = g.al + rc.off + e.alias; e = load_al_head<NT>(ep); ++reads; }
          if (biased) {
            const float u3 = (float)(o[3] >> 8) * (1.0f / 16777216.0f);
            const float thr = u3 * Q;
            if (e.id == prev) accepted = thr < inv_p;
            else if (thr < fminf(inv_q, 1.0f)) accepted = true;   // accepted whether or not x is in N(prev): no lookup
            else {
              // x in N(prev)?  On an undirected load this equals prev in N(x): probe the shorter sorted row
              bool in;
              if (g.ehash)                                  // one probe into the edge hash set: (prev -> x) exists?
                in = edge_exists(g.ehash, g.ehash_mask, (uint32_t)((int64_t)prev - g.vmin), (uint32_t)((int64_t)e.id - g.vmin));
              else {
                if (ep) { load_al_tail<NT>(ep, e); ep = nullptr; }     // the shorter-row choice needs the candidate's row
                if (g.symmetric && e.ndeg < rp.deg)
                  in = sorted_contains(g.sids + e.noff, e.ndeg, (uint32_t)((int64_t)prev - g.vmin));
                else
                  in = sorted_contains(g.sids + rp.off, rp.deg, (uint32_t)((int64_t)e.id - g.vmin));
              }
              accepted = thr < (in ? 1.0f : inv_q);
            }
            accepted = accepted || (t + 1u >= 65536u);
          }
        }
      }
      if (accepted) {
        if (ep) load_al_tail<NT>(ep, e);
        buf[s & (TILE - 1)] = e.id;
        if ((s & (TILE - 1)) == TILE - 1) {
          int32_t *dst = path + (s - (TILE - 1));
          if ((stride & 1) == 0) {                           // rows 8-byte aligned: 8-byte stores
#pragma unroll
            for (int c = 0; c < TILE; c += 2) {
              int2 v; v.x = buf[c]; v.y = buf[c + 1];
              *reinterpret_cast<int2 *>(dst + c) = v;
            }
          } else {                                           // back-to-back: the line is still in L2 when the last one lands
#pragma unroll
            for (int c = 0; c < TILE; ++c) dst[c] = buf[c];
          }
        }
        wprev_hint = e.wrev;
        prev = curr; rp = rc; curr = e.id;
        rc.off = e.noff; rc.deg = e.ndeg; rc.flags = e.nflags;
        ++s; ++len; t = 0;
      } else {
        ++t;
      }
    }
    for (int32_t t2 = len & ~(TILE - 1); t2 < len; ++t2) path[t2] = buf[t2 & (TILE - 1)];   // the partial last run
    for (int64_t t2 = len; t2 < stride; ++t2) path[t2] = -1;
    lens[wi] = len;
  }
  unsigned long long steps = len > 0 ? (unsigned long long)(len - 1) : 0ull;
  flush_counters(ctr, steps, dead, 0, 0, reads, fb);
  trials = wave_sum_u64(trials);
  if (lane_id() == 0 && trials) atomicAdd(&ctr->trials, trials);
}

// ---- unit hooks ------------------------------------------------------------------------------------------
__global__ void k_hook_pick(const Ent *row, int32_t deg, Bias b, float r, float *out_w, int64_t *index) {
  const int lane = lane_id();
  if (out_w)
    for (int32_t k = lane; k < deg; k += 64) out_w[k] = biased_weight(b, row[k].id, row[k].w);
  if (index) {
    unsigned f = 0;
    int32_t k = wave_pick(row, deg, b, r, f);
    if (lane == 0) *index = k;
  }
}
__global__ void k_hook_rng(uint32_t seed, const uint32_t *iter, const uint32_t *src, const uint32_t *step, int64_t n,
                           float *out) {
  RngSpec rng; rng.mode = 1; rng.const_r = 0.f; rng.seed = seed;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = draw_uniform(rng, iter[i], src[i], step[i]);
}
// cfo_pick on one row, one lattice draw per lane: position and loads issued.  pos = -1: the vertex is not in the graph or has no
// neighbours, -2: its row is irregular (never sampled through the compact records).
template <bool NT>
__global__ void k_hook_cfo_pick(GraphView g, int32_t vertex, const uint32_t *__restrict__ m, int64_t n, int32_t *__restrict__ pos,
                                int32_t *__restrict__ reads) {
  const int64_t slot = vertex_slot(vertex, g.rows, g.orig_id, g.n_slots, g.vmin);
  Row r; r.off = 0; r.deg = 0; r.flags = 0;
  if (slot < g.n_slots) r = g.rows[slot];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t k = r.deg <= 0 ? -1 : -2; unsigned rd = 0;
    if (r.deg > 0 && !(r.flags & ROW_IRREGULAR)) cfo_pick<NT>(g.cfo + r.off, r.deg, m[i], rd, k, g.cfo_reload != 0);
    pos[i] = k; reads[i] = (int32_t)rd;
  }
}

}  // namespace

void read_counters(srw_handle *h, srw_walk_stats *stats) {
  DevCounters c;
  SRW_HIP(hipMemcpyAsync(&c, h->counters.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  SRW_HIP(hipStreamSynchronize(h->stream));
#ifdef SRW_PHASE_TIMING
  {
    static const char *nm[10] = {"total", "prefix", "binned:ret-edges", "binned:P1", "binned:P2", "binned:W", "binned:search+resolve",
                                 "scan:fill", "scan:pass1", "scan:pass2"};
    fprintf(stderr, "[phase] wave-ms:");
    for (int i = 0; i < 10; ++i) fprintf(stderr, " %s %.0f", nm[i], (double)c.dbg[i] * 1024.0 / 100e3);
    fprintf(stderr, "\n[phase] W calls %llu elems %llu windows %llu | P1 calls %llu elems %llu | binned steps %llu\n", c.dbg[10], c.dbg[11],
            c.dbg[12], c.dbg[13], c.dbg[14], c.dbg[15]);
    {
      static const char *sn[12] = {"edge_table", "p1", "p2", "w", "p3", "scan", "prefix", "chain", "edge_mask", "-", "-", "-"};
      fprintf(stderr, "[phase] per-strategy wave-ms (whole step) / steps / us per step:");
      for (int i = 0; i < 12; ++i)
        if (c.strat[i]) fprintf(stderr, " %s %.0f / %llu / %.2f", sn[i], (double)c.dbg[24 + i] * 1024.0 / 100e3, c.strat[i],
                                (double)c.dbg[24 + i] * 1024.0 / 100.0 / (double)c.strat[i]);
      fprintf(stderr, "\n");
    }
    if (c.strat[SRW_STRAT_EDGE_TABLE])                   // the lean table kernel's own statistics (valid when it served the table steps)
      fprintf(stderr, "[lean] wave-ms: mask steps %.0f (%llu steps), table steps %.0f (%llu steps; %.0f with deg(prev) > 1024) | chunks %llu: "
              "no specials %llu, N(prev) staged %llu, hub bitmap %llu, edge hash %llu; candidates per chunk %.0f, rounds per chunk %.2f\n",
              (double)c.dbg[1] * 1024.0 / 100e3, c.strat[SRW_STRAT_EDGE_MASK], (double)c.dbg[2] * 1024.0 / 100e3, c.strat[SRW_STRAT_EDGE_TABLE],
              (double)c.dbg[3] * 1024.0 / 100e3, c.dbg[15], c.dbg[10], c.dbg[13], c.dbg[12], c.dbg[14],
              (double)c.dbg[11] / (double)std::max<unsigned long long>(c.dbg[15], 1), (double)c.dbg[16] / (double)std::max<unsigned long long>(c.dbg[15], 1));
    fprintf(stderr, "[phase] W detail wave-ms: wait-B %.0f clear+insert %.0f wait-A %.0f probe %.0f\n", (double)c.dbg[16] * 1024.0 / 100e3,
            (double)c.dbg[17] * 1024.0 / 100e3, (double)c.dbg[18] * 1024.0 / 100e3, (double)c.dbg[19] * 1024.0 / 100e3);
  }
#endif
  if (getenv("SRW_DEBUG_HANDOVER"))
    fprintf(stderr, "[handover] walkers %llu | q1 reasons: irregular row %llu, non-positive sum %llu, boundary draw %llu\n",
            c.strat[SRW_STAT_HANDED_OVER], c.why[0], c.why[1], c.why[2]);
  if (!stats) return;
  stats->n_steps = (int64_t)c.steps; stats->dead_ends = (int64_t)c.dead_ends;
  stats->sum_deg_curr = (int64_t)c.sum_deg_curr; stats->sum_deg_prev = (int64_t)c.sum_deg_prev;
  stats->ent_reads = (int64_t)c.ent_reads; stats->fallbacks = (int64_t)c.fallbacks; stats->trials = (int64_t)c.trials;
  for (int i = 0; i < 12; ++i) stats->strategy_steps[i] = (int64_t)c.strat[i];
  stats->edge_tables = (h->g.has_eb && h->g.use_eb) ? h->g.eb_tables : 0;
  stats->edge_table_bytes = (h->g.has_eb && h->g.use_eb) ? h->g.eb_bytes : 0;
}

void check_params(const srw_walk_params &P) {
  if (P.walk_length < 0) throw Error(SRW_ERR_INVALID, "walk_length must be >= 0");
  // --numWalks 0: the reference's `0 until numWalks` loop runs zero times and still writes an empty path/ + _SUCCESS
  if (P.num_walks < 0) throw Error(SRW_ERR_INVALID, "num_walks must be >= 0");
  if (P.rng_mode != SRW_RNG_CONST && P.rng_mode != SRW_RNG_PHILOX) throw Error(SRW_ERR_INVALID, "bad rng_mode");
  if (P.sampler != SRW_SAMPLER_REFERENCE && P.sampler != SRW_SAMPLER_ALIAS) throw Error(SRW_ERR_INVALID, "bad sampler");
  if (P.sampler == SRW_SAMPLER_ALIAS && P.rng_mode != SRW_RNG_PHILOX)
    throw Error(SRW_ERR_INVALID, "Mode A draws several uniforms per step: it needs SRW_RNG_PHILOX");
}

namespace {
struct LaunchInfo { int kind; int record_bytes; };

// Leaves no asynchronous work behind (copies into caller / pinned buffers, kernels writing staging buffers) when a
// pipelined entry point exits — normally or through an exception (I/O error in the writer, HIP error).
struct StreamDrain {
  srw_handle *h;
  explicit StreamDrain(srw_handle *hh) : h(hh) {}
  ~StreamDrain() {
    if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
  }
};

// Enqueue the walk kernel(s) of num_walks iterations starting at P.first_walk into d_paths / d_lens.
// Compacted ids (graph_build.hip:compact_ids): rank -> input id over the written part of every path, one wave per path.
__global__ void k_paths_to_ids(int32_t *__restrict__ paths, const int32_t *__restrict__ lens, int64_t n_walkers, int64_t stride,
                               const int32_t *__restrict__ orig_id) {
  const int lane = lane_id();
  for (int64_t w = blockIdx.x * (int64_t)(TPB / 64) + (threadIdx.x >> 6); w < n_walkers; w += (int64_t)gridDim.x * (TPB / 64)) {
    const int32_t len = lens[w];
    int32_t *row = paths + w * stride;
    for (int32_t k = lane; k < len; k += 64) row[k] = orig_id[row[k]];
  }
}

}  // namespace

void paths_to_ids(srw_handle *h, int32_t *d_paths, const int32_t *d_lens, int64_t n_walkers, int64_t stride) {
  const int64_t nb = std::min<int64_t>((n_walkers + TPB / 64 - 1) / (TPB / 64), (int64_t)h->n_cus * 32);
  hipLaunchKernelGGL(k_paths_to_ids, dim3((unsigned)nb), dim3(TPB), 0, h->stream, d_paths, d_lens, n_walkers, stride, (const int32_t *)h->g.orig_id.p);
  SRW_HIP(hipGetLastError());
}

namespace {
LaunchInfo launch_walk(srw_handle *h, const srw_walk_params &P, int32_t num_walks, int32_t first_walk, int32_t *d_paths,
                       int32_t *d_lens) {
  Graph &g = h->g;
  { const char *e = getenv("SRW_DEBUG_CHAIN_DEG"); g.dbg_chain_deg = e && *e ? atoi(e) : 0; }      // tests: every table step on a long row is a "tie"
  hipStream_t st = h->stream;
  // the walkers' start vertices: every present vertex, or the caller's list (srw_set_sources) in its order
  const int32_t *verts = h->start_verts();
  const int64_t n_verts = h->walkers_per_iteration();
  const int64_t n_walkers = (int64_t)num_walks * n_verts;
  const bool alias = P.sampler == SRW_SAMPLER_ALIAS;
  bool first_order_compact = false;
  const bool first_order = !alias && (P.p == 1.0f && P.q == 1.0f) && !(P.flags & SRW_WALK_FORCE_GENERAL);
  RngSpec rng; rng.mode = P.rng_mode; rng.const_r = P.const_r; rng.seed = P.seed;
  GraphView gv = g.view();
  if (alias) {
    int64_t blocks = (n_walkers + TPB - 1) / TPB;
    const size_t al_bytes = (size_t)g.n_entries * sizeof(AEnt);
    // cached loads by default: the accepted record's link is a second load of the same sector and should hit L2
    // (measured at weighted RMAT-24, p=.25 q=4: 5.4 G steps/s cached vs 5.3 G nontemporal; p=4 q=.5: 18.9 vs 15.6)
    (void)al_bytes;
    const bool nt = (P.flags & SRW_WALK_NT_LOADS) != 0;
    if (nt)
      hipLaunchKernelGGL(k_walk_alias<true>, dim3((unsigned)blocks), dim3(TPB), 0, st, gv, verts, n_verts, n_walkers,
                         P.walk_length, first_walk, P.seed, P.p, P.q, d_paths, d_lens, h->counters.p);
    else
      hipLaunchKernelGGL(k_walk_alias<false>, dim3((unsigned)blocks), dim3(TPB), 0, st, gv, verts, n_verts, n_walkers,
                         P.walk_length, first_walk, P.seed, P.p, P.q, d_paths, d_lens, h->counters.p);
  } else if (first_order) {
    int64_t blocks = (n_walkers + TPB - 1) / TPB;
    // Load policy for the linked records: once the table is far larger than L2 + Infinity Cache (32 + 256 MiB) a
    // record is used once per fetch, and an L1-bypassing load avoids pulling its whole 128-B line (measured on
    // MI355X: RMAT-26 19.6 -> 27.1 G steps/s); cache-resident tables keep the default policy (RMAT-20 35 vs 29).
    const size_t fo_bytes = (size_t)g.n_entries * sizeof(FoEnt);
    const bool nt = (P.flags & SRW_WALK_NT_LOADS) ? true
                    : (P.flags & SRW_WALK_CACHED_LOADS) ? false : fo_bytes > ((size_t)2 << 30);
    const int occ = (P.flags >> 8) & 0xF;   // experiment switch: requested min waves/SIMD (0 = compiler's choice)
    // 16-byte compact records: Philox draws only (p = m * 2^-24), and only if the whole graph qualified at build time
    const bool compact = g.has_cfo && P.rng_mode == SRW_RNG_PHILOX && !(P.flags & SRW_WALK_NO_COMPACT);
    first_order_compact = compact;
    const bool legacy_flush = (P.flags & SRW_WALK_LEGACY_FLUSH) != 0;
#define SRW_LAUNCH_FO_W(NTV, MW, CP, LG)                                                                            \
  hipLaunchKernelGGL((k_walk_first_order<NTV, MW, CP, LG>), dim3((unsigned)blocks), dim3(TPB), 0, st, gv, verts,       \
                     n_verts, n_walkers, P.walk_length, first_walk, rng, d_paths, d_lens, h->counters.p)
#define SRW_LAUNCH_FO(NTV, MW, CP)                                                                                  \
  do { if (legacy_flush) SRW_LAUNCH_FO_W(NTV, MW, CP, true); else SRW_LAUNCH_FO_W(NTV, MW, CP, false); } while (0)
    if (compact) {
      const bool ntc = (P.flags & SRW_WALK_NT_LOADS) ? true : (P.flags & SRW_WALK_CACHED_LOADS) ? false
                       : (size_t)g.n_entries * sizeof(CfoEnt) > ((size_t)2 << 30);
      if (ntc) SRW_LAUNCH_FO(true, 1, true); else SRW_LAUNCH_FO(false, 1, true);
    } else if (nt) { if (occ == 8) SRW_LAUNCH_FO(true, 8, false); else if (occ == 7) SRW_LAUNCH_FO(true, 7, false); else SRW_LAUNCH_FO(true, 1, false); }
    else    { if (occ == 8) SRW_LAUNCH_FO(false, 8, false); else if (occ == 7) SRW_LAUNCH_FO(false, 7, false); else SRW_LAUNCH_FO(false, 1, false); }
#undef SRW_LAUNCH_FO
#undef SRW_LAUNCH_FO_W
  } else {
    // persistent waves taking walkers from a cursor: enough blocks to fill every CU at the kernel's occupancy
    int64_t blocks = std::min<int64_t>((n_walkers * 64 + TPB - 1) / TPB, (int64_t)h->n_cus * 8);
    h->walk_cursor.ensure(2);
    SRW_HIP(hipMemsetAsync(h->walk_cursor.p, 0, 2 * sizeof(unsigned long long), st));
    const int32_t tune = (int32_t)(((P.flags >> 12) & 15) | ((P.flags & SRW_WALK_NO_BINNED) ? 16 : 0));
    // every (prev -> curr) pair has a table: the lean kernel walks, the general one only redoes what it hands over
    const bool lean = gv.eb_off && g.eb_complete && P.q != 1.0f && tune == 0 && !getenv("SRW_NO_LEAN_KERNEL");
    // p != 1, q == 1: one walker per lane over the first-order guide table + exact prefix sums + return-edge positions
    const bool q1 = P.q == 1.0f && P.p != 1.0f && P.rng_mode == SRW_RNG_PHILOX && g.has_cfo && g.has_pq && g.has_rev &&
                    g.pq_bad_rows == 0 && tune == 0 && !(P.flags & SRW_WALK_NO_PREFIX) && !getenv("SRW_NO_Q1_KERNEL");
    const int32_t *todo = nullptr;
    // Steps whose draw sits on a CDF boundary (the per-lane / lean kernels cannot decide them): recorded by those kernels, resolved by
    // the chain kernels (the whole GPU + one short pass per record, in passes that fit the quotient scratch) and taken from there by
    // k_walk_general when it redoes the walker — one wave alone took up to ~50 ms for the chain over a 10^6-candidate row
    const int32_t *todo_tie = nullptr; const ChainRec *tie_list = nullptr; const SWalker *tie_out = nullptr;
    TieSink tie; tie.hdr = nullptr; tie.recs = nullptr; tie.list = nullptr; tie.cur = nullptr; tie.todo_tie = nullptr;
    ChainBufs cb;
    const bool ties = lean && P.rng_mode == SRW_RNG_PHILOX && !getenv("SRW_NO_TIE_KERNELS");   // (the per-lane q == 1 kernel: measured, no gain — the records cost its registers what the redo saves)
    if (q1 || lean) h->walk_todo.ensure(2 * (size_t)n_walkers);          // handed-over walkers | their tie records
    if (ties) {
      cb = chain_bufs(h);
      SRW_HIP(hipMemsetAsync(cb.tie_cur, 0, 48, st));                                   // cursor array + chunk header
      SRW_HIP(hipMemsetAsync(cb.tie_out, 0xFF, (size_t)CHAIN_CAP * sizeof(SWalker), st));   // kind = -1: not resolved
      tie.hdr = cb.tie_hdr; tie.recs = cb.tie_recs; tie.list = cb.list; tie.cur = cb.tie_cur + 2;
      tie.todo_tie = h->walk_todo.p + n_walkers;
    }
    auto resolve_ties = [&]() {
      if (!ties) return;
      ShardIO io; io.recv = reinterpret_cast<const char *>(cb.tie_hdr); io.chunk_bytes = 0; io.cap_w = CHAIN_CAP; io.cap_r = 0;
      io.world = 1; io.rank = 0; io.batch = 0x7FFFFFFF; io.pt = nullptr; io.lens = nullptr; io.n_rows = 0;      // lw = the iteration's offset
      srw_walk_params Pc = P; Pc.first_walk = first_walk;
      static const int n_pass = getenv("SRW_TIE_PASSES") ? std::max(1, atoi(getenv("SRW_TIE_PASSES"))) : 8;
      for (int pass = 0; pass < n_pass; ++pass)          // (a pass with nothing left is five empty launches)
        enqueue_chain(h, cb, gv, io, Pc, 0, 0, rng, cb.tie_out, -1, cb.tie_cur, cb.tie_skip, cb.tie_cur + 3);
      todo_tie = tie.todo_tie; tie_list = cb.list; tie_out = cb.tie_out;
    };
    if (q1) {
      const int64_t qb = (n_walkers + TPB - 1) / TPB;
      const uint32_t q1_max_ret = getenv("SRW_Q1_MAX_RET") ? (uint32_t)atoi(getenv("SRW_Q1_MAX_RET")) : 16u;   // more parallel return edges: the whole wave takes the step
      if ((size_t)g.n_entries * sizeof(CfoEnt) > ((size_t)2 << 30))
        hipLaunchKernelGGL(k_walk_q1<true>, dim3((unsigned)qb), dim3(TPB), 0, st, gv, verts, n_verts, n_walkers, P.walk_length,
                           first_walk, rng, P.p, d_paths, d_lens, h->counters.p, h->walk_todo.p, h->walk_cursor.p + 1, q1_max_ret);
      else
        hipLaunchKernelGGL(k_walk_q1<false>, dim3((unsigned)qb), dim3(TPB), 0, st, gv, verts, n_verts, n_walkers, P.walk_length,
                           first_walk, rng, P.p, d_paths, d_lens, h->counters.p, h->walk_todo.p, h->walk_cursor.p + 1, q1_max_ret);
      todo = h->walk_todo.p;
    }
    if (lean) {
      int64_t lb = std::min<int64_t>((n_walkers * 64 + TPB - 1) / TPB, (int64_t)h->n_cus * 16);
      TabArgs ta;
      ta.g = gv; ta.verts = verts; ta.n_verts = n_verts; ta.n_walkers = n_walkers; ta.L = P.walk_length; ta.first_walk = first_walk;
      ta.rng = rng; ta.p = P.p; ta.q = P.q; ta.paths = d_paths; ta.lens = d_lens; ta.ctr = h->counters.p; ta.cursor = h->walk_cursor.p;
      ta.todo = h->walk_todo.p; ta.todo_n = h->walk_cursor.p + 1; ta.tie = tie;
      // One walker per LANE (walk_lanes.hip, mode 2: table steps per lane, the rest served by the wave) where the standing tables have
      // chunks of 64 candidates — config 3: 585 against 602 ms per iteration, directed RMAT-23 ef 27 (p = 4, q = .5): 132 against 206 ms;
      // one walker per WAVE (k_walk_tables) where a graph that fills the GPU left only chunks of >= 256: every table step would be served
      // (config 5's stand-in: 4.13 against 3.34 s) — profiles/r06_lane_kernel.md.  SRW_TABLE_LANES=<mode> forces the lane kernel (bit 0: whole
      // rows per lane, bit 1: table steps per lane), -1 the wave kernel.
      const int lanes = getenv("SRW_TABLE_LANES") ? atoi(getenv("SRW_TABLE_LANES")) : (gv.ebp.min_sh <= 6 ? 2 : -1);
      if (lanes >= 0) {
        launch_walk_tables_lanes(ta, gv.bf_off != nullptr, lanes, getenv("SRW_LANE_CSH") ? atoi(getenv("SRW_LANE_CSH")) : 6, h->n_cus, st);
      } else if (gv.bf_off) {
        hipLaunchKernelGGL((k_walk_tables<true>), dim3((unsigned)lb), dim3(TPB), 0, st, ta);
      } else {
        hipLaunchKernelGGL((k_walk_tables<false>), dim3((unsigned)lb), dim3(TPB), 0, st, ta);
      }
      SRW_HIP(hipMemsetAsync(h->walk_cursor.p, 0, sizeof(unsigned long long), st));
      todo = h->walk_todo.p;
      resolve_ties();
    }
    hipLaunchKernelGGL(k_walk_general, dim3((unsigned)blocks), dim3(TPB), 0, st, gv, verts, n_verts, n_walkers,
                       P.walk_length, first_walk, rng, P.p, P.q, d_paths, d_lens, h->counters.p, h->walk_cursor.p, tune, todo,
                       h->walk_cursor.p + 1, todo_tie, tie_list, tie_out);
  }
  SRW_HIP(hipGetLastError());
  LaunchInfo li;
  li.kind = alias ? 3 : first_order ? 1 : 2;
  li.record_bytes = first_order_compact ? 16 : (first_order || alias) ? 32 : 0;
  // compacted ids: the kernels walked over ranks; the paths leave with the ids of the input
  if (g.compact && n_walkers > 0) paths_to_ids(h, d_paths, d_lens, n_walkers, (int64_t)P.walk_length + 2);
  return li;
}

void prepare_tables(srw_handle *h, const srw_walk_params &P) {
  // SRW_TIMING: where the cold start of a call goes, phase by phase (each phase synchronises the stream when timing is on)
  const bool timing = getenv("SRW_TIMING") != nullptr;
  auto t_phase = std::chrono::steady_clock::now();
  auto phase = [&](const char *name) {
    if (!timing) return;
    (void)hipStreamSynchronize(h->stream);
    const auto t = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t - t_phase).count();
    if (ms >= 20.0) fprintf(stderr, "[timing] prepare_tables: %s %.0f ms\n", name, ms);
    t_phase = t;
  };
  const bool alias = P.sampler == SRW_SAMPLER_ALIAS;
  const bool first_order = !alias && (P.p == 1.0f && P.q == 1.0f) && !(P.flags & SRW_WALK_FORCE_GENERAL);
  if (first_order) build_first_order_tables(h, P.rng_mode != SRW_RNG_PHILOX || (P.flags & SRW_WALK_NO_COMPACT));
  else build_membership(h);                           // sorted rows: general and alias kernels only
  // p != 1, q == 1 (k_walk_q1): the compact first-order records (guide + linked rows) and the return-edge positions
  if (!alias && !first_order && P.q == 1.0f && P.p != 1.0f && P.rng_mode == SRW_RNG_PHILOX && h->cfg.world == 1 &&
      !(P.flags & (SRW_WALK_NO_PREFIX | SRW_WALK_NO_COMPACT)) && !getenv("SRW_NO_Q1_KERNEL")) {
    build_first_order_tables(h, false);
    build_rev_table(h);
  }
  phase("membership / first-order tables / return edges");
  if (alias) build_alias_tables(h);
  phase("alias tables");
  const bool general = !alias && !first_order;
  // optional accelerators, most valuable first (each one skips itself when HBM is short):
  // exact base prefix sums for the search samplers ...
  if (general && !(P.p == 1.0f && P.q == 1.0f) && !(P.flags & SRW_WALK_NO_PREFIX)) build_pq_tables(h, P.p, P.q);
  else if (general) h->g.has_pq = false;
  // ... the edge hash set answers "x in N(prev)?" in one probe: Mode A's rejection test, and the general kernel's
  // candidate-by-candidate membership (small rows, the located chunk of the binned search)
  bool want_ehash = P.q != 1.0f && !(P.flags & SRW_WALK_NO_EDGE_HASH) && (alias || (general && h->cfg.world == 1));
  // neighbor-set bitmaps of the hub rows: the general kernel's "x in N(prev)" for steps that come from a hub
  const bool want_hub = general && P.q != 1.0f && h->cfg.world == 1 && !(P.flags & SRW_WALK_NO_HUB_BITMAPS);
  const bool want_eb = general && P.q != 1.0f && h->cfg.world == 1 && h->g.has_pq && !(P.flags & SRW_WALK_NO_EDGE_TABLES) &&
                       !(P.flags & SRW_WALK_NO_BINNED);
  const int eb_mode = (P.flags & SRW_WALK_EDGE_TABLES_ALL) ? 1 : 0;
  phase("prefix sums of the (p, q) base weights");
  if (want_eb) build_unit_ids(h);                     // unit-weight graphs: 4-byte ids for the table steps (before the tables are sized)
  phase("unit-weight ids");
  const char *env_hub = getenv("SRW_HUB_BUDGET_GB"), *env_cap = getenv("SRW_EB_CHUNKS");
  // The edge hash (8 B x 2-3 per entry) against table resolution: when a COMPLETE 64-chunk set of per-edge tables fits only
  // without the hash, the hash goes — the located chunks' probes of a long non-hub N(prev) fall back to the sorted row, and
  // every step still gains from chunks half as long (config 5's stand-in: 34 GB of hash; 32 chunks + hash 1.67e8 steps/s,
  // 32 chunks without 1.56e8, 64 chunks without 2.0e8 — s68, s69).
  // ---- what HBM is spent on, in this order -------------------------------------------------------------------------
  // A table step is bound by the memory requests it issues (profiles/r04_request_attribution.md), and what removes requests is table
  // resolution: (1) a COMPLETE set (a cut set sends its uncovered steps to the on-the-fly samplers of the monolithic kernel) with as many
  // chunks per table as fit (256 / 128 / 64 / 32), (2) the smallest chunk (64 / 128 / 256 candidates), (3) chunk masks for the rows up
  // to 16 384 / 4 096 candidates whose N(prev) is too long for the LDS staging, (4) finer tables (up to 4 096 / 1 024 / 512 chunks) for
  // the unmasked pairs with a long N(prev).  The edge hash (8 B x 2-3 per entry: one probe per candidate of a located chunk that has
  // neither mask nor staged N(prev) nor hub bitmap) is kept only when dropping it would not buy a finer set — without it the long rows
  // get their neighbor-set filters (4 B per entry) in front of the sorted rows (config 5's stand-in: 34 GB of hash; s68, s69, r04 s109).
  // The hub bitmaps take what is left (at least 16 GB are set aside for them).
  bool drop_ehash = false;
  size_t hub_cap = want_eb ? (size_t)16 << 30 : (size_t)64 << 30;
  size_t table_cap_used = 0;
  int eb_cap = EB_BINS;
  if (env_hub && *env_hub) hub_cap = (size_t)(atof(env_hub) * (double)((size_t)1 << 30));
  if (env_cap && *env_cap) eb_cap = atoi(env_cap);
  struct TabPlan { int cap = 0, min_sh = 8, cm = 0, fine = 0, ratio = 0; size_t need = 0; bool complete = false; };
  auto finer = [](const TabPlan &a, const TabPlan &b) {      // a strictly finer than b
    if (a.complete != b.complete) return a.complete;
    if (a.cap != b.cap) return a.cap > b.cap;
    if (a.min_sh != b.min_sh) return a.min_sh < b.min_sh;
    return std::min(a.cm, 16384) > std::min(b.cm, 16384);          // (long masks, the finer tables of the unmasked pairs and the mask ratio are refinements: not worth the hash — config 3: ratio 16
                                 //  without the hash 771 ms per iteration, ratio 4 with it 711 ms, r04 s112)
  };
  // what the walk itself allocates after the tables: one call's paths and lengths (+ hand-over lists, chain scratch, the build's HBM-scratch bins)
  size_t reserve = (size_t)P.num_walks * (size_t)h->walkers_per_iteration() * ((size_t)P.walk_length + 3) * 4 + ((size_t)8 << 30);
  if (reserve > ((size_t)64 << 30)) reserve = (size_t)64 << 30;      // (srw_walk_to_host / _and_save stream one iteration at a time)
  if (const char *r = getenv("SRW_EB_RESERVE_GB"); r && *r) reserve = (size_t)(atof(r) * (double)((size_t)1 << 30));
  h->g.eb_reserve = reserve;
  const int64_t job_walks = std::max<int64_t>(h->planned_walks > 0 ? h->planned_walks : 10, P.num_walks);   // srw_plan_walks
  std::map<std::tuple<int, int, int, int, int>, size_t> size_cache;
  auto set_size = [&](int cap, int sh, int cm, int fine, int ratio = 0) {   // bytes of the complete set under this geometry (one pass over the entries; cached)
    Graph &g = h->g;
    const auto key = std::make_tuple(cap, sh, cm, fine, ratio);
    auto it = size_cache.find(key);
    if (it != size_cache.end()) return it->second;
    g.eb_min_sh_sel = sh; g.eb_cm_sel = cm; g.eb_fine_cap_sel = fine; g.eb_cm_ratio_sel = ratio;
    const size_t n = edge_tables_full_bytes(h, eb_mode, cap);
    if (getenv("SRW_TIMING")) fprintf(stderr, "[timing] table plan: %d chunks of >= %d, masks <= %d (ratio %d), fine %d: %.1f GB\n", cap, 1 << sh, cm, ratio, fine, (double)n / 1e9);
    size_cache[key] = n;
    return n;
  };
  auto plan_tables = [&](size_t free_b) {                    // the finest geometry whose complete set fits into free_b next to the reserve and the bitmaps' minimum
    TabPlan t;
    const size_t ceiling = (size_t)230 << 30;                 // (eb_off counts 64-byte units in 32 bits: 256 GiB)
    auto fits = [&](size_t n, size_t margin) { return n > 0 && n < ceiling && free_b > n + reserve + margin; };
    const bool fixed_cap = env_cap && *env_cap;
    if (fixed_cap) { t.cap = eb_cap; t.need = set_size(t.cap, 8, 0, 0); t.complete = fits(t.need, (size_t)8 << 30); }
    else
      for (int c : {256, 128, 64, 32}) {
        const size_t n = set_size(c, 8, 0, 0);
        if (fits(n, (size_t)(c > 64 ? 40 : 8) << 30)) { t.cap = c; t.need = n; t.complete = true; break; }
      }
    if (!t.complete) { if (!t.cap) { t.cap = EB_BINS; t.need = set_size(t.cap, 8, 0, 0); } return t; }
    if (eb_mode) return t;
    if (!getenv("SRW_EB_MIN_SH"))
      for (int sh : {6, 7}) {
        const size_t n = set_size(t.cap, sh, 0, 0);
        if (fits(n, (size_t)40 << 30)) { t.min_sh = sh; t.need = n; break; }
      }
    // chunk masks: every row up to 16 384 candidates (4 096 if memory is short).  LONG masks (round 6: rows beyond 16 384 candidates for the
    // pairs with a long N(prev) — the hub -> hub pairs whose located chunks probe prev's bitmap once per candidate) are built when asked for
    // (SRW_EB_CM_MAX > 16 384) but never planned: at config 3 they need +100 GB up to 32 768 candidates (no change in the iteration: 588 ms),
    // +150 GB up to 131 072, +184 GB for every row — the probes come from the longest rows (profiles/r06_long_masks.md)
    if (!getenv("SRW_EB_CM_MAX"))
      for (int cm : {16384, 4096}) {
        const size_t n = set_size(t.cap, t.min_sh, cm, 0);
        if (fits(n, (size_t)24 << 30)) { t.cm = cm; t.need = n; break; }
      }
    // Finer tables for the unmasked pairs with a long N(prev).  Up to 512 chunks they fill the wave's LDS bins like every other table and
    // cost nothing to build (config 3: +40 ms, +15 GB, 643 -> 602 ms per iteration); beyond that the bins live in an HBM scratch
    // (+1.6 - 8 s by box and 40 GB more for 602 -> 573 ms): only for a job long enough to pay for them — srw_plan_walks,
    // profiles/r05_table_build.md.
    if (!getenv("SRW_EB_FINE_CAP"))
      for (int fc : {4096, 1024, 512}) {
        if (fc <= t.cap) break;
        if (fc > BIN_CAP && job_walks < 64) continue;
        const size_t n = set_size(t.cap, t.min_sh, t.cm, fc);
        if (fits(n, (size_t)24 << 30)) { t.fine = fc; t.need = n; break; }
      }
    if (t.cm && !getenv("SRW_EB_CM_RATIO"))
      for (int ratio : {16, 4}) {
        const size_t n = set_size(t.cap, t.min_sh, t.cm, t.fine, ratio);
        if (fits(n, (size_t)24 << 30)) { t.ratio = ratio; t.need = n; break; }
      }
    return t;
  };
  TabPlan plan;
  bool standing = false;
  if (want_eb) {
    Graph &g = h->g;
    uint32_t pb, qb; memcpy(&pb, &P.p, 4); memcpy(&qb, &P.q, 4);
    standing = g.has_eb && !g.eb_sharded && g.eb_pbits == pb && g.eb_qbits == qb && g.eb_mode == eb_mode && (!want_hub || g.has_hub);
    if (standing) {
      drop_ehash = g.eb_no_ehash;                                  // standing tables: as they were built, with the bitmaps they were built with
      eb_cap = g.eb_cap;
      if (want_hub) hub_cap = g.hub_budget_cap;
    } else {
      uint64_t slots = 1024;
      while (slots < (uint64_t)g.n_entries + (uint64_t)g.n_entries / 2) slots <<= 1;      // build_edge_hash's sizing
      const size_t eh_bytes = (size_t)slots * 8;
      size_t free_b = 0, total_b = 0;
      SRW_HIP(hipMemGetInfo(&free_b, &total_b));
      free_b += g.hub_bm.n * sizeof(uint32_t) + g.eb_bins.n * sizeof(double) + g.em_bits.n * sizeof(uint32_t) + g.eb_off.n * sizeof(uint32_t);
      if (g.has_ehash) free_b += g.ehash.n * sizeof(uint64_t);     // free_b: with neither hash nor tables nor bitmaps nor filters
      if (g.has_bf) free_b += (g.bf_off.n + g.bf_bits.n) * sizeof(uint32_t);
      const size_t filters = (size_t)g.n_entries * 4 + (size_t)g.n_slots * 4;
      const TabPlan with = (want_ehash && free_b > eh_bytes) ? plan_tables(free_b - eh_bytes) : TabPlan();
      const TabPlan without = plan_tables(free_b > filters ? free_b - filters : 0);
      // equal plans: with chunk masks the few probes left are one request each in the hash (config 3: 711 ms with it, 771 ms without, r04 s112);
      // without masks every located chunk probes all of its candidates, and the filters answer most of those from L2 (config 5's stand-in, the
      // same 128 x 256 plan: 4 560 ms without the hash, 5 555 ms with it, r04 u2)
      drop_ehash = want_ehash && (finer(without, with) || (!finer(with, without) && without.complete && without.cm == 0 && !eb_mode));
      plan = (want_ehash && !drop_ehash) ? with : without;
      if (getenv("SRW_TIMING"))
        fprintf(stderr, "[timing] table plan: %.1f GB free; with the edge hash (%.1f GB): %s %d chunks of >= %d, masks <= %d (ratio %d), fine %d (%.1f GB); without: %s %d chunks of >= %d, "
                "masks <= %d (ratio %d), fine %d (%.1f GB) -> %s\n", (double)free_b / 1e9, (double)eh_bytes / 1e9, with.complete ? "complete" : "cut", with.cap, 1 << with.min_sh, with.cm, with.ratio, with.fine,
                (double)with.need / 1e9, without.complete ? "complete" : "cut", without.cap, 1 << without.min_sh, without.cm, without.ratio, without.fine, (double)without.need / 1e9,
                drop_ehash ? "the hash goes" : "the hash stays");
      eb_cap = plan.cap ? plan.cap : eb_cap;
      g.eb_min_sh_sel = plan.min_sh; g.eb_cm_sel = plan.cm; g.eb_fine_cap_sel = plan.fine; g.eb_cm_ratio_sel = plan.ratio;
      if (plan.need > ((size_t)160 << 30)) table_cap_used = (size_t)230 << 30;
      const size_t used = (drop_ehash || !want_ehash) ? filters : eh_bytes;
      const size_t keep = plan.need + reserve + ((size_t)8 << 30) + used;
      if (!(env_hub && *env_hub) && want_hub && plan.need > 0 && free_b > keep + ((size_t)16 << 30))
        hub_cap = std::min<size_t>(free_b - keep, (size_t)96 << 30);
    }
  }
  if (want_eb && want_ehash && getenv("SRW_EB_DROP_EHASH")) drop_ehash = true;      // tests: the traded configuration on any graph
  if (drop_ehash) {
    want_ehash = false;
    if (h->g.has_ehash) { h->g.ehash.release(); h->g.has_ehash = false; }
  }
  phase("table plan (sizing passes)");
  if (want_ehash) build_edge_hash(h);
  h->g.use_ehash = want_ehash;
  phase("edge hash");
  // no edge hash for the table steps (traded above, or not wanted): the long rows' neighbor-set filters answer most of the
  // located chunks' probes from L2 (config 5's stand-in: 2.0e8 -> 2.73e8 steps/s, 3 GB).  With the hash they are not worth
  // their registers (config 3: -1 ... -4 %): k_walk_tables<false>.
  if (want_eb && !want_ehash && !getenv("SRW_NO_ROW_FILTERS")) build_row_filters(h);
  phase("row filters");
  if (want_hub) build_hub_bitmaps(h, ((P.flags >> 15) & 1) ? 1 : 1024, hub_cap);
  h->g.use_hub = want_hub;
  phase("hub bitmaps");
  // ... and, last (they take what HBM is left), the per-edge bias tables: the most expensive (prev, curr) pairs get
  // their N(prev) ∩ N(curr) corrections precomputed once per (p, q) instead of once per visit
  if (want_eb) {
    h->g.eb_budget_gb = table_cap_used ? (table_cap_used >> 30) : drop_ehash ? 200 : 160;
    // The sizing above works from hipMemGetInfo; if an allocation of the build fails all the same (fragmentation), the
    // walk goes on with a coarser set, or with none (the on-the-fly samplers) — an optional accelerator never fails a walk.
    for (int attempt = 0; attempt < 2; ++attempt) {
      try { build_edge_tables(h, P.p, P.q, eb_mode, attempt == 0 ? eb_cap : 32); break; }
      catch (const Error &e) {
        // a mapping call of the progressively mapped table buffer refused for another reason than memory (vm_buf.h): once more, the
        // buffer as one hipMalloc — an optional accelerator never fails a walk
        const bool remap = e.code == SRW_ERR_HIP && vm_buf_broken().load() && attempt == 0 && std::string(e.what()).find("mapping the table buffer") != std::string::npos;
        if (e.code != SRW_ERR_NOMEM && !remap) throw;
        (void)hipGetLastError();
        (void)hipStreamSynchronize(h->stream);          // (segments of the build may be running over the chunks that did get mapped)
        if (remap) {
          h->g.eb_bins.release(); h->g.em_bits.release(); h->g.has_eb = false;
          if (getenv("SRW_TIMING")) fprintf(stderr, "[timing] per-edge tables: %s — once more with one allocation\n", e.what());
          attempt = -1;                                   // (the loop's ++ makes it attempt 0 again, now without the mapped range)
          continue;
        }
        Graph &g = h->g;
        g.eb_bins.release(); g.em_bits.release(); g.has_eb = false; g.eb_complete = false; g.eb_tables = 0; g.eb_bytes = 0;
        h->g.eb_budget_gb = 160; g.eb_min_sh_sel = 8; g.eb_cm_sel = 0; g.eb_fine_cap_sel = 0; g.eb_cm_ratio_sel = 0;
        if (getenv("SRW_TIMING")) fprintf(stderr, "[timing] per-edge tables: %s — %s\n", e.what(), attempt == 0 && eb_cap > 32 ? "retrying with 32 chunks" : "walking without them");
        if (eb_cap <= 32) break;
      }
    }
    h->g.eb_no_ehash = drop_ehash;
  }
  h->g.use_eb = want_eb;
  phase("per-edge tables");
}
double timed_prepare_tables(srw_handle *h, const srw_walk_params &P) {   // builders synchronise the stream themselves
  const auto t0 = std::chrono::steady_clock::now();
  prepare_tables(h, P);
  SRW_HIP(hipStreamSynchronize(h->stream));
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

void run_walk(srw_handle *h, const srw_walk_params &P, srw_walk_stats *stats) {
  Graph &g = h->g;
  if (!g.loaded) throw Error(SRW_ERR_INVALID, "no graph loaded");
  if (h->cfg.world != 1) throw Error(SRW_ERR_INVALID, "srw_walk needs a whole-graph handle (world == 1); use srw_shard_*");
  check_params(P);
  hipStream_t st = h->stream;
  const int64_t n_walkers = (int64_t)P.num_walks * h->walkers_per_iteration();
  if (n_walkers >= ((int64_t)1 << 31)) throw Error(SRW_ERR_INVALID, "more than 2^31 walkers in one call: lower num_walks");
  const int32_t stride = P.walk_length + 2;
  if (n_walkers == 0) {   // empty graph, empty source list or num_walks == 0: nothing to walk
    h->res.n_walkers = 0; h->res.stride = stride; h->res.valid = true;
    if (stats) { memset(stats, 0, sizeof(*stats)); }
    return;
  }
  const double setup_ms = timed_prepare_tables(h, P);
  h->res.valid = false;
  h->res.paths.ensure((size_t)n_walkers * stride);
  h->res.lens.ensure((size_t)n_walkers);
  h->res.n_walkers = n_walkers; h->res.stride = stride;
  h->counters.ensure(1);
  SRW_HIP(hipMemsetAsync(h->counters.p, 0, sizeof(DevCounters), st));
  SRW_HIP(hipEventRecord(h->ev0, st));
  LaunchInfo li = launch_walk(h, P, P.num_walks, P.first_walk, h->res.paths.p, h->res.lens.p);
  SRW_HIP(hipEventRecord(h->ev1, st));
  srw_walk_stats local;
  srw_walk_stats *s = stats ? stats : &local;
  memset(s, 0, sizeof(*s));
  read_counters(h, s);
  float ms = 0.f;
  SRW_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  s->kernel_ms = ms; s->setup_ms = setup_ms; s->n_walkers = n_walkers; s->kernel_kind = li.kind; s->record_bytes = li.record_bytes;
  h->res.valid = true;
}

// numWalks iterations streamed to the host: kernel of iteration i on the compute stream, D2H of iteration i-1 on the
// copy stream, two staging buffers; events order "kernel done -> copy" and "copy done -> buffer reuse".
void run_walk_to_host(srw_handle *h, const srw_walk_params &P, int32_t *paths, int32_t *lens, srw_walk_stats *stats) {
  Graph &g = h->g;
  if (!g.loaded) throw Error(SRW_ERR_INVALID, "no graph loaded");
  if (h->cfg.world != 1) throw Error(SRW_ERR_INVALID, "srw_walk_to_host needs a whole-graph handle (world == 1)");
  check_params(P);
  hipStream_t st = h->stream;
  const int64_t nv = h->walkers_per_iteration();   // walkers of one iteration: present vertices, or the source list
  if (nv >= ((int64_t)1 << 31)) throw Error(SRW_ERR_INVALID, "too many walkers per iteration");
  const int32_t stride = P.walk_length + 2;
  if (nv == 0 || P.num_walks == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return; }
  const double setup_ms = timed_prepare_tables(h, P);
  if (!h->copy_stream) SRW_HIP(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) {
    h->stage_paths[i].ensure((size_t)nv * stride);
    h->stage_lens[i].ensure((size_t)nv);
    if (!h->stage_done[i]) SRW_HIP(hipEventCreateWithFlags(&h->stage_done[i], hipEventDisableTiming));
    if (!h->kernel_done[i]) SRW_HIP(hipEventCreateWithFlags(&h->kernel_done[i], hipEventDisableTiming));
  }
  h->res.valid = false;
  h->counters.ensure(1);
  StreamDrain drain(h);
  SRW_HIP(hipMemsetAsync(h->counters.p, 0, sizeof(DevCounters), st));
  SRW_HIP(hipEventRecord(h->ev0, st));
  LaunchInfo li{0, 0};
  for (int32_t it = 0; it < P.num_walks; ++it) {
    const int b = it & 1;
    if (it >= 2) SRW_HIP(hipStreamWaitEvent(st, h->stage_done[b], 0));           // buffer b was copied out
    li = launch_walk(h, P, 1, P.first_walk + it, h->stage_paths[b].p, h->stage_lens[b].p);
    SRW_HIP(hipEventRecord(h->kernel_done[b], st));
    SRW_HIP(hipStreamWaitEvent(h->copy_stream, h->kernel_done[b], 0));
    SRW_HIP(hipMemcpyAsync(paths + (size_t)it * nv * stride, h->stage_paths[b].p, (size_t)nv * stride * 4,
                           hipMemcpyDeviceToHost, h->copy_stream));
    SRW_HIP(hipMemcpyAsync(lens + (size_t)it * nv, h->stage_lens[b].p, (size_t)nv * 4, hipMemcpyDeviceToHost, h->copy_stream));
    SRW_HIP(hipEventRecord(h->stage_done[b], h->copy_stream));
  }
  SRW_HIP(hipEventRecord(h->ev1, st));
  SRW_HIP(hipStreamSynchronize(h->copy_stream));
  srw_walk_stats local;
  srw_walk_stats *s = stats ? stats : &local;
  memset(s, 0, sizeof(*s));
  read_counters(h, s);
  float ms = 0.f;
  SRW_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  s->kernel_ms = ms; s->setup_ms = setup_ms; s->n_walkers = (int64_t)P.num_walks * nv; s->kernel_kind = li.kind; s->record_bytes = li.record_bytes;
}

// randomWalk + save fused and streamed (Main.doRandomWalk, M/Main.scala:53-62): the paths never exist as a whole on
// the host.  Per walk iteration: kernel on the compute stream -> D2H into a pinned ring slot on the copy stream ->
// the host formats and appends the PREVIOUS iteration's slice to <output>/path/part-* while the GPU works on this one.
void run_walk_and_save(srw_handle *h, const srw_walk_params &P, const char *output_dir, int n_parts, bool write_crc,
                       srw_walk_stats *stats, int64_t *dead_per_iter) {
  Graph &g = h->g;
  if (!g.loaded) throw Error(SRW_ERR_INVALID, "no graph loaded");
  if (h->cfg.world != 1) throw Error(SRW_ERR_INVALID, "srw_walk_and_save needs a whole-graph handle (world == 1)");
  check_params(P);
  hipStream_t st = h->stream;
  const int64_t nv = h->walkers_per_iteration();   // walkers of one iteration: present vertices, or the source list
  const int32_t stride = P.walk_length + 2;
  PathWriter writer(output_dir, n_parts, (int64_t)P.num_walks * nv, write_crc);   // fails first if <output>/path exists
  if (nv == 0 || P.num_walks == 0) { writer.close(); if (stats) memset(stats, 0, sizeof(*stats)); return; }   // empty part-00000 + _SUCCESS
  const double setup_ms = timed_prepare_tables(h, P);
  if (!h->copy_stream) SRW_HIP(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  const size_t need = (size_t)nv * stride * 4;
  bool device_format = (P.flags & SRW_WALK_DEVICE_FORMAT) != 0;
  const size_t cap = format_capacity(nv, stride, g.id_lo, g.id_hi);
  if (device_format) {        // two text slots in HBM: fall back to the host formatter when they do not fit
    size_t free_b = 0, total_b = 0;
    SRW_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t have = h->fmt_text[0].n + h->fmt_text[1].n;
    const size_t slots = P.num_walks > 1 ? 2 : 1;
    if (slots * cap > have && free_b < slots * cap - have + need * slots + ((size_t)4 << 30)) device_format = false;
  }
  const int n_slots = P.num_walks > 1 ? 2 : 1;             // (a single iteration never touches the second staging / text slot: tens of GB at the headline's size)
  for (int i = 0; i < 2; ++i) {
    if (i < n_slots) { h->stage_paths[i].ensure((size_t)nv * stride); h->stage_lens[i].ensure((size_t)nv); }
    if (!h->stage_done[i]) SRW_HIP(hipEventCreateWithFlags(&h->stage_done[i], hipEventDisableTiming));
    if (!h->kernel_done[i]) SRW_HIP(hipEventCreateWithFlags(&h->kernel_done[i], hipEventDisableTiming));
    // pinned ring: the ids only travel to the host when the host formats them; the lengths always do (dead-end counts)
    if (!device_format && h->pin_cap < need) {
      if (h->pin_paths[i]) (void)hipHostFree(h->pin_paths[i]);
      h->pin_paths[i] = nullptr;
      SRW_HIP(hipHostMalloc((void **)&h->pin_paths[i], need ? need : 4, hipHostMallocDefault));
    }
    if (h->pin_lens_cap < (size_t)nv) {
      if (h->pin_lens[i]) (void)hipHostFree(h->pin_lens[i]);
      h->pin_lens[i] = nullptr;
      SRW_HIP(hipHostMalloc((void **)&h->pin_lens[i], (size_t)nv * 4 + 4, hipHostMallocDefault));
    }
  }
  if (!device_format) h->pin_cap = std::max(h->pin_cap, need);
  h->pin_lens_cap = std::max(h->pin_lens_cap, (size_t)nv);
  h->res.valid = false;
  h->counters.ensure(1);
  StreamDrain drain(h);
  SRW_HIP(hipMemsetAsync(h->counters.p, 0, sizeof(DevCounters), st));
  SRW_HIP(hipEventRecord(h->ev0, st));
  LaunchInfo li{0, 0};
  if (device_format) {
    // Device-side formatter (path_format.hip): the GPU turns iteration `it` into text while the host copies out and
    // writes the text of iteration `it - 1`; the host never touches the ids.
    for (int i = 0; i < n_slots; ++i) { h->fmt_text[i].ensure(cap); h->fmt_len[i].ensure((size_t)nv + 1); h->fmt_off[i].ensure((size_t)nv + 1); }
    const int32_t N = P.num_walks;
    auto launch = [&](int32_t it) {
      const int b = it & 1;
      li = launch_walk(h, P, 1, P.first_walk + it, h->stage_paths[b].p, h->stage_lens[b].p);
      format_paths_device(h, h->stage_paths[b].p, h->stage_lens[b].p, nv, stride, h->fmt_len[b].p, h->fmt_off[b].p,
                          h->fmt_text[b].p);
      SRW_HIP(hipEventRecord(h->kernel_done[b], st));
    };
    // The text leaves the device in slices of whole lines through the ring of pinned buffers (path_format.hip:drain_text): the next
    // slices are copied while the writer's threads put the earlier ones into their part files.
    const size_t slice_cap = text_slice_cap(stride, cap);
    ensure_pinned_text(h, slice_cap, (size_t)nv + 1);
    launch(0);
    if (N > 1) launch(1);
    for (int32_t k = 0; k < N; ++k) {
      const int b = k & 1;
      const auto tk0 = std::chrono::steady_clock::now();
      SRW_HIP(hipEventSynchronize(h->kernel_done[b]));                      // walk + format of iteration k done
      if (getenv("SRW_TIMING")) fprintf(stderr, "[timing] walk_and_save: waited %.0f ms for walk + format of iteration %d\n",
                                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tk0).count(), k);
      unsigned long long *off = h->pin_off[b];
      SRW_HIP(hipMemcpyAsync(off, h->fmt_off[b].p, ((size_t)nv + 1) * 8, hipMemcpyDeviceToHost, h->copy_stream));
      SRW_HIP(hipMemcpyAsync(h->pin_lens[b], h->stage_lens[b].p, (size_t)nv * 4, hipMemcpyDeviceToHost, h->copy_stream));
      SRW_HIP(hipStreamSynchronize(h->copy_stream));
      drain_text(h, writer, h->fmt_text[b].p, off, nv, slice_cap, [&] { if (k + 2 < N) launch(k + 2); });   // every byte of device slot b is out: reuse it
      if (dead_per_iter) {
        int64_t dead = 0;
        for (int64_t i = 0; i < nv; ++i) dead += (h->pin_lens[b][i] >= 2 && h->pin_lens[b][i] < stride);
        dead_per_iter[k] = dead;
      }
    }
    SRW_HIP(hipEventRecord(h->ev1, st));
    writer.close();
    srw_walk_stats local;
    srw_walk_stats *s = stats ? stats : &local;
    memset(s, 0, sizeof(*s));
    read_counters(h, s);
    float ms = 0.f;
    SRW_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    s->kernel_ms = ms; s->setup_ms = setup_ms; s->n_walkers = (int64_t)P.num_walks * nv; s->kernel_kind = li.kind; s->record_bytes = li.record_bytes;
    return;
  }
  auto consume = [&](int32_t it) {      // host side of iteration `it`: wait for its slice, format + append
    const int b = it & 1;
    SRW_HIP(hipEventSynchronize(h->stage_done[b]));
    if (dead_per_iter) {
      int64_t dead = 0;
      for (int64_t i = 0; i < nv; ++i) dead += (h->pin_lens[b][i] >= 2 && h->pin_lens[b][i] < stride);
      dead_per_iter[it] = dead;
    }
    writer.append(h->pin_paths[b], h->pin_lens[b], nv, stride);
  };
  for (int32_t it = 0; it < P.num_walks; ++it) {
    const int b = it & 1;
    // device staging slot b is free once its previous copy finished; the pinned slot b once the host consumed it
    if (it >= 2) SRW_HIP(hipStreamWaitEvent(st, h->stage_done[b], 0));
    li = launch_walk(h, P, 1, P.first_walk + it, h->stage_paths[b].p, h->stage_lens[b].p);
    SRW_HIP(hipEventRecord(h->kernel_done[b], st));
    if (it >= 2) consume(it - 2);                                   // frees pinned slot b before it is overwritten
    SRW_HIP(hipStreamWaitEvent(h->copy_stream, h->kernel_done[b], 0));
    SRW_HIP(hipMemcpyAsync(h->pin_paths[b], h->stage_paths[b].p, need, hipMemcpyDeviceToHost, h->copy_stream));
    SRW_HIP(hipMemcpyAsync(h->pin_lens[b], h->stage_lens[b].p, (size_t)nv * 4, hipMemcpyDeviceToHost, h->copy_stream));
    SRW_HIP(hipEventRecord(h->stage_done[b], h->copy_stream));
  }
  SRW_HIP(hipEventRecord(h->ev1, st));
  for (int32_t it = std::max(0, P.num_walks - 2); it < P.num_walks; ++it) consume(it);
  writer.close();
  srw_walk_stats local;
  srw_walk_stats *s = stats ? stats : &local;
  memset(s, 0, sizeof(*s));
  read_counters(h, s);
  float ms = 0.f;
  SRW_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  s->kernel_ms = ms; s->setup_ms = setup_ms; s->n_walkers = (int64_t)P.num_walks * nv; s->kernel_kind = li.kind; s->record_bytes = li.record_bytes;
}

void hook_sample(srw_handle *h, const float *w, int64_t n, float r, int64_t *index) {
  hook_second_order(h, 1.0f, 1.0f, 0, nullptr, 0, nullptr, w, n, r, nullptr, index);
}

void hook_second_order(srw_handle *h, float p, float q, int32_t prev_id, const int32_t *prev_ids, int64_t n_prev,
                       const int32_t *curr_ids, const float *curr_w, int64_t n, float r, float *out_w,
                       int64_t *index) {
  if (n <= 0) { if (index) *index = -1; return; }
  if (n > 0x7FFFFFFF || n_prev > 0x7FFFFFFF) throw Error(SRW_ERR_INVALID, "list too long");
  hipStream_t st = h->stream;
  std::vector<Ent> row((size_t)n);
  int32_t vmin = prev_id;
  for (int64_t k = 0; k < n; ++k) { row[k].id = curr_ids ? curr_ids[k] : (int32_t)k; row[k].w = curr_w[k]; vmin = std::min(vmin, row[k].id); }
  for (int64_t k = 0; k < n_prev; ++k) vmin = std::min(vmin, prev_ids[k]);
  std::vector<uint32_t> sp((size_t)n_prev);
  for (int64_t k = 0; k < n_prev; ++k) sp[k] = (uint32_t)((int64_t)prev_ids[k] - vmin);
  std::sort(sp.begin(), sp.end());
  DevBuf<Ent> d_row; DevBuf<uint32_t> d_sp; DevBuf<float> d_w; DevBuf<int64_t> d_idx;
  d_row.alloc((size_t)n); d_sp.alloc((size_t)n_prev); d_w.alloc((size_t)n); d_idx.alloc(1);
  SRW_HIP(hipMemcpyAsync(d_row.p, row.data(), (size_t)n * sizeof(Ent), hipMemcpyHostToDevice, st));
  if (n_prev) SRW_HIP(hipMemcpyAsync(d_sp.p, sp.data(), (size_t)n_prev * 4, hipMemcpyHostToDevice, st));
  Bias b; b.p = p; b.q = q; b.prev = prev_id; b.second_order = (prev_ids != nullptr) || (p != 1.0f) || (q != 1.0f);
  b.need_member = b.second_order && q != 1.0f; b.prev_sids = d_sp.p; b.prev_deg = (int32_t)n_prev; b.vmin = vmin;
  hipLaunchKernelGGL(k_hook_pick, dim3(1), dim3(64), 0, st, d_row.p, (int32_t)n, b, r, out_w ? d_w.p : nullptr,
                     index ? d_idx.p : nullptr);
  SRW_HIP(hipGetLastError());
  if (out_w) SRW_HIP(hipMemcpyAsync(out_w, d_w.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (index) SRW_HIP(hipMemcpyAsync(index, d_idx.p, 8, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
}

void hook_rng(srw_handle *h, uint32_t seed, const uint32_t *iter, const uint32_t *src, const uint32_t *step,
              int64_t n, float *out) {
  if (n <= 0) return;
  hipStream_t st = h->stream;
  DevBuf<uint32_t> a, b, c; DevBuf<float> o;
  a.alloc((size_t)n); b.alloc((size_t)n); c.alloc((size_t)n); o.alloc((size_t)n);
  SRW_HIP(hipMemcpyAsync(a.p, iter, (size_t)n * 4, hipMemcpyHostToDevice, st));
  SRW_HIP(hipMemcpyAsync(b.p, src, (size_t)n * 4, hipMemcpyHostToDevice, st));
  SRW_HIP(hipMemcpyAsync(c.p, step, (size_t)n * 4, hipMemcpyHostToDevice, st));
  int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(k_hook_rng, dim3(blocks), dim3(256), 0, st, seed, a.p, b.p, c.p, n, o.p);
  SRW_HIP(hipGetLastError());
  SRW_HIP(hipMemcpyAsync(out, o.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
}

void hook_cfo_pick(srw_handle *h, int32_t vertex, const uint32_t *m, int64_t n, int32_t *pos, int32_t *reads) {
  if (n <= 0) return;
  Graph &g = h->g;
  if (!g.loaded) throw Error(SRW_ERR_INVALID, "no graph loaded");
  if (h->cfg.world > 1) throw Error(SRW_ERR_INVALID, "srw_cfo_pick: a sharded handle (world > 1) has no whole-graph compact table");
  for (int64_t i = 0; i < n; ++i)
    if (m[i] >> 24) throw Error(SRW_ERR_INVALID, "srw_cfo_pick: a draw is not below 2^24");
  build_first_order_tables(h, false);
  if (!g.has_cfo) throw Error(SRW_ERR_INVALID, "srw_cfo_pick: this graph has no compact first-order table (a record needs an escape)");
  hipStream_t st = h->stream;
  DevBuf<uint32_t> dm; DevBuf<int32_t> dp, dr;
  dm.alloc((size_t)n); dp.alloc((size_t)n); dr.alloc((size_t)n);
  SRW_HIP(hipMemcpyAsync(dm.p, m, (size_t)n * 4, hipMemcpyHostToDevice, st));
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  const GraphView gv = g.view();
  // both load policies of the walk give the same picks; the nontemporal one is the headline kernel's
  hipLaunchKernelGGL(k_hook_cfo_pick<true>, dim3(blocks), dim3(256), 0, st, gv, vertex, dm.p, n, dp.p, dr.p);
  SRW_HIP(hipGetLastError());
  SRW_HIP(hipMemcpyAsync(pos, dp.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipMemcpyAsync(reads, dr.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  if (pos[0] == -1) throw Error(SRW_ERR_INVALID, "srw_cfo_pick: the vertex is not in the graph or has no neighbours");
  if (pos[0] == -2) throw Error(SRW_ERR_INVALID, "srw_cfo_pick: the vertex's row is irregular (it is not sampled through the compact records)");
}

}  // namespace srw
