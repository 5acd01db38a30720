// chain_kernels.hip — the exact chain for the steps whose draw sits on a CDF boundary (gfx950): k_chain_setup, k_chain_d, k_chain_scan,
// k_chain_u, k_chain_seq and their host side.  The sharded super-step lists its ties per super-step (shard_kernels.hip), the whole-graph
// table kernels all ties of a launch at once (walk_kernels.hip: TieSink); both reach them through enqueue_chain.
#include <cstdlib>

#include "engine.h"
#include "sampling.h"
#include "walk_shared.h"

namespace srw {
namespace {
// ---- the exact chain for the table steps whose draw sits on a CDF boundary ---------------------------------------------
// RandomSample.sample's running sum (RandomSample.scala:18-22) is sequential by nature, but only its ADDITIONS are: the
// quotients fl(w'_k / S) — the entry loads, the membership probes, the divides: what costs — are independent.  So:
//   k_chain_setup  one thread: row length, scratch offset and first work unit of every listed record (records whose
//                  quotients do not fit the scratch array go to the general step)
//   k_chain_d      the whole GPU: one wave per work unit of 256 candidates computes their quotients into the scratch array
//   k_chain_seq    one wave per record: the chain over the stored quotients, 1024 per round (chain_round_fast: one integer
//                  sum per round while no rounding tie / binade crossing / answer is in it), next round prefetched
// ~3 000 ties per iteration at config 3's size, each up to a million candidates long: one wave alone took 10-40 ms for one.
// pass_cur (whole-graph walks: ALL ties of a launch are listed at once — several GB of quotients at config 3): the records are taken
// in several passes of the chain kernels, each one as many as fit the scratch array; *pass_cur = the first record not taken yet.
__global__ void k_chain_setup(GraphView g, ShardIO io, const ChainRec *__restrict__ list, unsigned long long *cursor /* [1] todo_n, [2] chain_n */,
                              ChainMeta *__restrict__ meta, uint32_t *__restrict__ totals /* [0] work units, [1] records */, long long d_cap,
                              uint32_t *__restrict__ todo, unsigned long long *pass_cur) {
  __shared__ uint32_t pre[SHARD_MAX_WORLD + 1];
  __shared__ int32_t degs[CHAIN_CAP];
  shard_in_prefix(io, pre);
  const unsigned long long n_all = cursor[2];
  const uint32_t n = (uint32_t)(n_all < (unsigned long long)CHAIN_CAP ? n_all : (unsigned long long)CHAIN_CAP);
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {       // the rows' lengths, all lanes (one dependent pair of loads each)
    const SWalker wk = shard_in_record(io, pre, list[i].ri);
    degs[i] = g.rows[(int64_t)wk.curr - g.vmin].deg;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint32_t start = pass_cur ? (uint32_t)(*pass_cur < (unsigned long long)n ? *pass_cur : (unsigned long long)n) : 0u;
  uint32_t next_start = start;
  bool stopped = false;
  long long off = 0; uint32_t units = 0;
  for (uint32_t i = 0; i < n; ++i) {
    ChainMeta m; m.d_off = off; m.deg = 0; m.u_off = units;          // deg 0: not in this pass
    if (i >= start && !stopped) {
      const int32_t deg = degs[i];
      if (off + (long long)deg <= d_cap) {
        m.deg = deg; off += (long long)((deg + 255) & ~255); units += (uint32_t)((deg + 255) >> 8); next_start = i + 1;
      } else if (!pass_cur) todo[atomicAdd(cursor + 1, 1ull)] = list[i].ri;     // scratch full: the general step
      else if (off == 0) next_start = i + 1;                                   // longer than the whole scratch array: stays unresolved
      else stopped = true;                                                     // the next pass starts here
    }
    meta[i] = m;
  }
  totals[0] = units; totals[1] = n;
  if (pass_cur) *pass_cur = next_start;
}
__global__ __launch_bounds__(TPB) void k_chain_d(GraphView g, ShardIO io, float p, float q, const ChainRec *__restrict__ list,
                                                 const ChainMeta *__restrict__ meta, const uint32_t *__restrict__ totals, double *__restrict__ D,
                                                 ChainUnits cu) {
  __shared__ uint32_t pre[SHARD_MAX_WORLD + 1];
  shard_in_prefix(io, pre);
  const int lane = lane_id();
  const uint32_t n_units = totals[0], n = totals[1];
  const uint32_t gw = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6), nw = gridDim.x * (TPB / 64);
  uint32_t i = 0;
  for (uint32_t u = gw; u < n_units; u += nw) {
    ChainMeta m = meta[i];                                 // the record unit u belongs to (u grows: i only moves forward)
    while (u >= m.u_off + (uint32_t)((m.deg + 255) >> 8) && i + 1 < n) m = meta[++i];
    const int32_t base4 = (int32_t)(u - m.u_off) * 256;
    const SWalker wk = shard_record_uniform(io, pre, list[i].ri);
    const Row r = uniform_row(g.rows[(int64_t)wk.curr - g.vmin]);
    const bool need = q != 1.0f;                           // q == 1 (k_sh_step_q1's ties): only the return edges are biased
    Row mr; mr.off = 0; mr.deg = 0; mr.flags = 0;
    if (need) mr = uniform_row(g.mrows[(int64_t)wk.prev - g.vmin]);
    Bias b;
    b.p = p; b.q = q; b.prev = wk.prev; b.second_order = true; b.need_member = need; b.vmin = g.vmin;
    b.prev_sids = need ? g.msids + mr.off : nullptr; b.prev_deg = mr.deg; b.prev_hub = mr.flags >> ROW_HUB_SHIFT;
    Member cm; cm.mode = need ? 1 : 0; cm.bm = nullptr; cm.seg_base = 0;
    cm.hub = (b.prev_hub && g.hub_bm) ? g.hub_bm + (int64_t)(b.prev_hub - 1) * g.hub_words : nullptr;
    cm.ehash = g.ehash; cm.ehash_mask = g.ehash_mask;
    if (!cm.hub && !g.ehash && g.bf_off && mr.deg >= BF_MIN_DEG) {
      const uint32_t bo = g.bf_off[(int64_t)wk.prev - g.vmin];
      if (bo != BF_NONE) { cm.bf = g.bf_bits + bo; cm.bf_nw = bf_words(mr.deg); }
    }
    double d4[4];
    chain_quotients4(g.ent + r.off, r.deg, base4, b, list[i].S, &cm, d4);
    double *out = D + m.d_off + base4;
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) out[uu * 64 + lane] = d4[uu];          // (padding up to the unit's 256 slots holds 0.0)
    const double us = wave_sum_f64((d4[0] + d4[1]) + (d4[2] + d4[3]));    // approximate: only places the unit in a binade (k_chain_scan)
    if (lane == 0) cu.usum[u] = us;
  }
}
// One wave per record: the approximate accumulator at every unit's start and end (a plain scan of the units' sums) names the
// binade the unit is expected to run in (-1: the two ends differ).  A guess only: k_chain_seq checks it against the exact accumulator.
__global__ __launch_bounds__(TPB) void k_chain_scan(const ChainMeta *__restrict__ meta, const uint32_t *__restrict__ totals, ChainUnits cu) {
  const int lane = lane_id();
  const uint32_t i = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (i >= totals[1]) return;
  const ChainMeta m = meta[i];
  if (m.deg == 0) return;
  const int32_t nu = (m.deg + 255) >> 8;
  double carry = 0.0;
  for (int32_t base = 0; base < nu; base += 64) {
    const int32_t j = base + lane;
    const double v = j < nu ? cu.usum[m.u_off + j] : 0.0;
    double incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const double t = __shfl_up(incl, off); if (lane >= off) incl += t; }
    const double a0 = carry + (incl - v), a1 = carry + incl;
    const unsigned long long b0 = (unsigned long long)__double_as_longlong(a0), b1 = (unsigned long long)__double_as_longlong(a1);
    const int e0 = (int)((b0 >> 52) & 0x7FFull), e1 = (int)((b1 >> 52) & 0x7FFull);
    if (j < nu) cu.ue[m.u_off + j] = (e0 == e1 && e0 != 0 && e0 != 0x7FF && !(b0 >> 63)) ? e0 : -1;
    carry += readlane_f64(incl, 63);
  }
}
// The whole GPU, one wave per unit: the unit's 256 quotients as ONE integer increment of the accumulator in the guessed binade
// (chain_round_fast's argument: without a rounding tie the maps N -> N + c commute); CHAIN_UNIT_SLOW when an element sits on a
// tie or would leave the binade by itself, or the unit has no guess.
constexpr unsigned long long CHAIN_UNIT_SLOW = ~0ull;
__global__ __launch_bounds__(TPB) void k_chain_u(const uint32_t *__restrict__ totals, const double *__restrict__ D, ChainUnits cu) {
  const int lane = lane_id();
  const uint32_t n_units = totals[0];
  const uint32_t gw = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6), nw = gridDim.x * (TPB / 64);
  for (uint32_t u = gw; u < n_units; u += nw) {
    const int e = cu.ue[u];
    double d4[4];
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) d4[uu] = D[(long long)u * 256 + uu * 64 + lane];
    unsigned long long loc = 0ull; bool odd = e < 0;
    if (e >= 0) {
#pragma unroll
      for (int uu = 0; uu < 4; ++uu) {
        unsigned long long c0 = 0ull, c1 = 0ull;
        chain_elem_map(d4[uu], e - 1023, c0, c1);
        odd |= (c0 != c1) || (c0 >> 53);
        loc += c0;
      }
    }
    const bool slow = __any(odd);
    const unsigned long long tot = wave_sum_u64(loc);
    if (lane == 0) cu.utot[u] = (slow || (tot >> 53)) ? CHAIN_UNIT_SLOW : tot;
  }
}
// One wave per record, 64 units (16 384 quotients) per iteration: lane l holds unit j + l's integer increment; a wave scan gives the
// accumulator after each unit, exactly, while the guessed binade is the accumulator's and the sum stays inside it.  The first unit
// that is slow (a tie inside, no / wrong guess), would leave the binade or reaches p is evaluated element by element
// (chain_group64: the reference's additions) — the first ~20 units of a row (the accumulator climbs through the small binades),
// one per binade crossing afterwards, and the answer's unit.  A 10^6-candidate row: ~64 iterations + ~25 slow units, where
// one integer sum per 1024 quotients took ~1000 dependent rounds (2.7 ms per super-step on RMAT-24's hubs).
__global__ __launch_bounds__(TPB) void k_chain_seq(GraphView g, ShardIO io, int32_t first_walk, int32_t step, int32_t last, RngSpec rng,
                                                   const ChainRec *__restrict__ list, const ChainMeta *__restrict__ meta,
                                                   const uint32_t *__restrict__ totals, const double *__restrict__ D, ChainUnits cu,
                                                   SWalker *__restrict__ scratch, DevCounters *ctr, int strat) {
  __shared__ uint32_t pre[SHARD_MAX_WORLD + 1];
  shard_in_prefix(io, pre);
  const int lane = lane_id();
  const uint32_t i = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (i >= totals[1]) return;
  const ChainMeta m = meta[i];
  if (m.deg == 0) return;                                 // handed to the general step by k_chain_setup
  const uint32_t ri = list[i].ri;
  const SWalker wk = shard_record_uniform(io, pre, ri);
  const Row r = uniform_row(g.rows[(int64_t)wk.curr - g.vmin]);
  const uint32_t iter = (uint32_t)(first_walk + wk.lw % io.batch);
  if (list[i].pad) step = (int32_t)list[i].pad;           // whole-graph walks: every tie has its own step (TieSink)
  const double p = (double)draw_uniform(rng, iter, (uint32_t)__builtin_amdgcn_readfirstlane(rng_source(g, wk.src)), (uint32_t)step);
  const double *d = D + m.d_off;
  const int32_t nu = (r.deg + 255) >> 8;
  double acc = 0.0;
  int32_t k_hit = -1, j = 0;
  [[maybe_unused]] unsigned n_slow = 0;
  while (j < nu && k_hit < 0) {
    const unsigned long long ab = (unsigned long long)__double_as_longlong(acc);
    const int ea = (int)((ab >> 52) & 0x7FFull);
    int f = 0;                                            // units absorbed by this iteration
    if (!(ea == 0 || ea == 0x7FF || (ab >> 63))) {
      const unsigned long long N0 = (ab & ((1ull << 52) - 1ull)) | (1ull << 52);
      const bool valid = j + lane < nu;
      const unsigned long long tot = valid ? cu.utot[m.u_off + j + lane] : 0ull;
      const int eg = valid ? cu.ue[m.u_off + j + lane] : ea;
      const bool slow = valid && (tot == CHAIN_UNIT_SLOW || eg != ea);
      unsigned long long incl = slow ? 0ull : tot;        // (lanes behind the first stop are not used)
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const unsigned long long t = shfl_up_u64(incl, off); if (lane >= off) incl += t; }
      const unsigned long long N = N0 + incl;
      const double a = __longlong_as_double((long long)(((unsigned long long)ea << 52) | (N & ((1ull << 52) - 1ull))));
      const unsigned long long stop = __ballot(slow || (valid && (N >= (1ull << 53) || !(a < p))));
      const int n_valid = min(64, nu - j);
      f = stop ? __ffsll((long long)stop) - 1 : n_valid;
      if (f > 0) acc = readlane_f64(a, f - 1);
      j += f;
      if (!stop) continue;
    }
    // unit j, element by element
    ++n_slow;
#pragma unroll 1
    for (int u = 0; u < 4; ++u) {
      const int32_t b0 = j * 256 + u * 64;
      if (b0 >= r.deg) break;                             // wave-uniform
      const int cnt = min(64, r.deg - b0);
      const double dv = lane < cnt ? d[b0 + lane] : 0.0;
      const int fh = chain_group64(acc, dv, cnt, p);
      if (fh >= 0) { k_hit = b0 + fh; break; }
    }
    ++j;
  }
  if (k_hit < 0) k_hit = 0;                               // edges.head (:24)
  if (lane == 0) {
    const int32_t next = g.ent[r.off + k_hit].id;
    SWalker nw = shard_advance(wk, step, next, last != 0);
    nw.pad0 = k_hit;
    scratch[ri] = nw;
    if (strat >= 0) {                                     // (whole-graph walks: k_walk_general counts the step it takes from here)
      atomicAdd(&ctr->steps, 1ull); atomicAdd(&ctr->fallbacks, 1ull);
      atomicAdd(&ctr->strat[SRW_STRAT_CHAIN], 1ull); atomicAdd(&ctr->strat[strat], 1ull);
    }
#ifdef SRW_PHASE_TIMING
    atomicAdd(&ctr->dbg[20], (unsigned long long)n_slow); atomicAdd(&ctr->dbg[21], (unsigned long long)nu);
#endif
  }
}
}  // namespace

ChainBufs chain_bufs(srw_handle *h) {
  static const long long d_cap = (long long)(getenv("SRW_CHAIN_SCRATCH_MB") ? atof(getenv("SRW_CHAIN_SCRATCH_MB")) : 512.0) * (1 << 20) / 8;
  const size_t n_units = (size_t)(d_cap / 256) + CHAIN_CAP;
  const size_t core = (size_t)CHAIN_CAP * (sizeof(ChainRec) + sizeof(ChainMeta)) + 64 + n_units * 24;
  const size_t tie = 64 + (size_t)CHAIN_CAP * (sizeof(WWalker) + sizeof(SWalker) + 4) + 64;
  h->chain_buf.ensure(core + tie);
  h->chain_d.ensure((size_t)d_cap);
  ChainBufs b;
  char *base = h->chain_buf.p;
  b.list = reinterpret_cast<ChainRec *>(base);
  b.meta = reinterpret_cast<ChainMeta *>(base + (size_t)CHAIN_CAP * sizeof(ChainRec));
  b.totals = reinterpret_cast<uint32_t *>(base + (size_t)CHAIN_CAP * (sizeof(ChainRec) + sizeof(ChainMeta)));
  char *ub = base + (size_t)CHAIN_CAP * (sizeof(ChainRec) + sizeof(ChainMeta)) + 64;
  b.cu.usum = reinterpret_cast<double *>(ub);
  b.cu.utot = reinterpret_cast<unsigned long long *>(ub + n_units * 8);
  b.cu.ue = reinterpret_cast<int32_t *>(ub + n_units * 16);
  b.D = h->chain_d.p; b.d_cap = d_cap;
  char *tb = base + ((core + 63) & ~(size_t)63);
  b.tie_cur = reinterpret_cast<unsigned long long *>(tb);                    // [0..3]: the cursor array of k_chain_setup ([1] skipped, [2] listed)
  b.tie_hdr = reinterpret_cast<uint32_t *>(tb + 32);                         // 16-byte chunk header, the records right behind it
  b.tie_recs = reinterpret_cast<WWalker *>(tb + 48);
  b.tie_out = reinterpret_cast<SWalker *>(tb + 48 + (size_t)CHAIN_CAP * sizeof(WWalker));
  b.tie_skip = reinterpret_cast<uint32_t *>(tb + 48 + (size_t)CHAIN_CAP * (sizeof(WWalker) + sizeof(SWalker)));
  return b;
}
// draws on a CDF boundary (listed by the step kernel at cursor[2]): quotients by the whole GPU, their units summarised, then one
// short sequential pass per record; what does not fit goes onto the todo list `skipped` (count at cursor[1]) — the general step's
void enqueue_chain(srw_handle *h, const ChainBufs &cb, const GraphView &gv, const ShardIO &io, const srw_walk_params &P, int32_t step, int32_t last,
                   const RngSpec &rng, SWalker *scratch, int strat, unsigned long long *cursor, uint32_t *skipped, unsigned long long *pass_cur) {
  hipStream_t st = h->stream;
  hipLaunchKernelGGL(k_chain_setup, dim3(1), dim3(256), 0, st, gv, io, cb.list, cursor, cb.meta, cb.totals, cb.d_cap, skipped, pass_cur);
  hipLaunchKernelGGL(k_chain_d, dim3(h->n_cus * 4), dim3(TPB), 0, st, gv, io, P.p, P.q, cb.list, cb.meta, cb.totals, cb.D, cb.cu);
  hipLaunchKernelGGL(k_chain_scan, dim3(CHAIN_CAP / (TPB / 64)), dim3(TPB), 0, st, cb.meta, cb.totals, cb.cu);
  hipLaunchKernelGGL(k_chain_u, dim3(h->n_cus * 4), dim3(TPB), 0, st, cb.totals, (const double *)cb.D, cb.cu);
  hipLaunchKernelGGL(k_chain_seq, dim3(CHAIN_CAP / (TPB / 64)), dim3(TPB), 0, st, gv, io, P.first_walk, step, last, rng, cb.list, cb.meta, cb.totals,
                     (const double *)cb.D, cb.cu, scratch, h->counters.p, strat);
}

}  // namespace srw
