// metapath.hip — walks whose steps are restricted to vertex types (gfx950): srw_vertex_types_set / srw_walk_metapath (include/stellar_rw.h).
// No reference counterpart: the reference walks homogeneous graphs.  The draw is still RandomSample.sample
// (M/algorithm/RandomSample.scala:12-25), applied to the SUBLIST of N(curr) whose vertices have the type the pattern names for the step.
//
//   k_entry_types     etype[e] = the type of adjacency entry e's vertex: the entry's id resolves to its slot (device_common.h:vertex_slot)
//                     and through ensure_vpos's array (sgns.hip) to its position in V, where the caller's types are indexed.  Built once
//                     per srw_vertex_types_set, 1 byte per entry: the walk then reads the candidates' types as a contiguous byte stream
//                     beside the row instead of one dependent byte gather per candidate.
//   k_walk_metapath   k_walk_general's outer structure (walk_kernels.hip): 256 threads, persistent waves taking the next walker from a
//                     cursor, one wave per walker, lane 0 writes path[s], tail and lens as there, counters flushed once per wave.  The
//                     pattern (<= 64 entries) travels in the kernel arguments.  Per step: wave_pick_typed.
//   wave_pick_typed   sampling.h:wave_pick_scan (mode 0) with "is a candidate" beside every weight.  Pass 1: four entries per lane per
//                     round of 256, w' = match ? w : 0, the match count (zero: the walk ends), the first matching position (the head
//                     fallback) and the certified-exact parallel sum — else the sequential f64 fold in row order (adding 0.0 for an
//                     entry that does not match is exact, so the fold over the row is the fold over the sublist).  Pass 2: the certified
//                     scan with tol_k = (k + 1) * 2^-51 * acc_k, k the ROW position (a bound no smaller than the sublist's); only a
//                     matching entry can be a hit.  A draw within rounding distance of a boundary, a sum without a certificate, a
//                     negative / NaN / Inf matching weight: the exact chain.
//   the chain         sampling.h:chain_round_fast over rounds of 256 (an entry that does not match is the quotient 0.0: absorbed
//                     exactly), and where a round has to be evaluated, group by group: the matching quotients of a group of 64 are
//                     moved to the group's first lanes in row order (one ds_permute) and handed to sampling.h:chain_group64 as they are
//                     — the chain runs over the sublist itself, so neither its acc == 0 single-addition branch nor an acc >= p that
//                     already holds at the row's head (u = 0) can return an entry that is no candidate.
// Rows of up to 64 entries take one round with the row in registers (pass 1, pass 2 and the chain read the same loads).
#include <algorithm>
#include <cstring>
#include <string>

#include "engine.h"
#include "sampling.h"
#include "walk_shared.h"

namespace srw {
namespace {

constexpr int MP_MAX = 64;                          // pattern entries at most
struct MetaPattern { int32_t m; int16_t t[MP_MAX]; };   // t[j]: 0 .. 255 a type, -1 any

__global__ __launch_bounds__(TPB) void k_entry_types(const Ent *__restrict__ ent, int64_t n_entries, const Row *__restrict__ rows, int64_t n_slots,
                                                     int32_t vmin, const int32_t *__restrict__ vpos, const uint8_t *__restrict__ vtypes,
                                                     uint8_t *__restrict__ etype) {
  for (int64_t e = blockIdx.x * (int64_t)TPB + threadIdx.x; e < n_entries; e += (int64_t)gridDim.x * TPB) {
    // (the ids inside the engine are slot + vmin, also on a graph with compacted ids: no orig_id look-up)
    const int64_t s = vertex_slot(ent[e].id, rows, nullptr, n_slots, vmin);
    const int32_t vp = s < n_slots ? vpos[s] : -1;
    etype[e] = vp >= 0 ? vtypes[vp] : (uint8_t)0;
  }
}

__device__ inline bool mp_match(int req, uint32_t t) { return req < 0 || (int)t == req; }

// chain_group64 over the candidates of one group of 64 entries (lane l: quotient d, cand = "entry l is a candidate"; lanes beyond
// the row are no candidates): a stable partition brings the candidates' quotients to lanes 0 .. c - 1 in row order.  -> the lane
// (= position inside the group) of the first candidate with acc >= p, or -1 (acc: the accumulator after the group's candidates).
__device__ inline int chain_group64_typed(double &acc, double d, bool cand, double p) {
  const int lane = lane_id();
  const unsigned long long m = __ballot(cand);
  const int c = __popcll(m);
  if (c == 0) return -1;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int dst = cand ? __popcll(m & below) : c + __popcll(~m & below);      // a permutation of the 64 lanes
  const uint64_t b = (uint64_t)__double_as_longlong(d);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_permute(dst << 2, (int)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_permute(dst << 2, (int)(uint32_t)(b >> 32));
  const int from = __builtin_amdgcn_ds_permute(dst << 2, lane);
  const int f = chain_group64(acc, __longlong_as_double((long long)(((uint64_t)hi << 32) | lo)), c, p);
  return f < 0 ? -1 : __builtin_amdgcn_readlane(from, f);
}

// The reference's chain over the sublist, 256 entries per round (wave_chain_pick's shape); head: the first candidate's position.
__device__ inline int32_t wave_chain_pick_typed(const GraphView &g, const Ent *row, const uint8_t *__restrict__ et, int32_t deg, int req, double p,
                                                double S, int32_t head) {
  const int lane = lane_id();
  double acc = 0.0;                                      // wave-uniform
  for (int32_t base4 = 0; base4 < deg; base4 += 256) {
    double d4[4]; bool c4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int32_t k = base4 + u * 64 + lane;
      d4[u] = 0.0; c4[u] = false;
      if (k < deg) {
        const Ent e = load_ent(g, row, k);
        c4[u] = mp_match(req, et[k]);
        if (c4[u]) d4[u] = (double)e.w / S;
      }
    }
    if (chain_round_fast<4>(acc, d4, p)) continue;       // (never with acc == 0: the first candidate is always added for real)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int32_t base = base4 + u * 64;
      if (base >= deg) break;                            // wave-uniform
      const int f = chain_group64_typed(acc, d4[u], c4[u], p);
      if (f >= 0) return base + f;
    }
  }
  return head;                                           // the sublist's head (:24)
}

// RandomSample.sample on the entries of the row whose type matches req (req < 0: all of them).  All 64 lanes call with identical
// arguments.  -> the chosen position in the row (wave-uniform), -1 when no entry matches; fallback = 1: the exact chain decided.
__device__ inline int32_t wave_pick_typed(const GraphView &g, const Row &rc, const uint8_t *__restrict__ etype, int req, float r, unsigned &fallback) {
  const int lane = lane_id();
  const Ent *row = g.ent + rc.off;
  const uint8_t *et = etype + rc.off;
  const int32_t deg = rc.deg;
  const double p = (double)r;
  if (deg <= 64) {
    // ---- one round, the row in registers ----
    Ent e; e.id = 0; e.w = 0.0f;
    bool cand = false;
    if (lane < deg) { e = load_ent(g, row, lane); cand = mp_match(req, et[lane]); }
    const unsigned long long cm = __ballot(cand);
    if (!cm) return -1;
    const int32_t head = __ffsll((long long)cm) - 1;
    const float w = cand ? e.w : 0.0f;
    SumCert cert;
    cert.add(w);
    const int emin = wave_min_i32(cert.emin), emax = wave_max_i32(cert.emax);
    const bool bad = __any(cert.bad) || __any(cand && !(w >= 0.0f));
    const bool exact = !bad && sum_is_exact(emin, emax, false, __popcll(cm));
    double S;
    if (exact) S = wave_sum_f64((double)w);
    else { S = 0.0; for (int i = 0; i < deg; ++i) S = S + readlane_f64((double)w, i); }
    const double d = cand ? (double)w / S : 0.0;
    if (exact) {
      const double acc = wave_incl_scan_f64(d);
      const double tol = (double)(lane + 1) * 0x1p-51 * acc;
      const unsigned long long open = __ballot(cand && !(acc + tol < p));     // candidates that are not a certain miss
      if (!open) return head;
      const int fl = __ffsll((long long)open) - 1;
      if (__builtin_amdgcn_readlane((int)(acc - tol >= p), fl)) return fl;
    }
    fallback = 1;
    double a0 = 0.0;
    const int f = chain_group64_typed(a0, d, cand, p);
    return f >= 0 ? f : head;
  }
  // ---- pass 1: candidates, head, S ----
  double part = 0.0;
  SumCert cert;
  bool neg = false;
  unsigned long long cnt = 0;
  int32_t first = 0x7FFFFFFF;
  for (int32_t base = 0; base < deg; base += 256) {
    const int32_t k0 = base + lane * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int32_t k = k0 + i;
      if (k < deg) {
        const Ent e = load_ent(g, row, k);
        const bool c = mp_match(req, et[k]);
        const float w = c ? e.w : 0.0f;
        part += (double)w;
        cert.add(w);
        neg |= c && !(w >= 0.0f);
        cnt += c ? 1ull : 0ull;
        first = c ? min(first, k) : first;
      }
    }
  }
  const unsigned long long n_cand = wave_sum_u64(cnt);
  if (n_cand == 0) return -1;
  const int32_t head = wave_min_i32(first);
  const int emin = wave_min_i32(cert.emin), emax = wave_max_i32(cert.emax);
  const bool bad = __any(cert.bad) || __any(neg);
  if (bad || !sum_is_exact(emin, emax, false, (int64_t)n_cand)) {
    double S = 0.0;                                      // foldLeft(0.0)(_ + w) over the sublist (:14): x + 0.0 == x for the others
    for (int32_t base = 0; base < deg; base += 64) {
      const int32_t k = base + lane;
      double wd = 0.0;
      if (k < deg) { const Ent e = load_ent(g, row, k); if (mp_match(req, et[k])) wd = (double)e.w; }
      const int n = min(64, deg - base);
      for (int i = 0; i < n; ++i) S = S + readlane_f64(wd, i);
    }
    fallback = 1;
    return wave_chain_pick_typed(g, row, et, deg, req, p, S, head);
  }
  const double S = wave_sum_f64(part);
  // ---- pass 2: certified scan ----
  double carry = 0.0;
  for (int32_t base = 0; base < deg; base += 256) {
    const int32_t k0 = base + lane * 4;
    double l[4];
    bool c4[4];
    double run = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int32_t k = k0 + i;
      double d = 0.0;
      c4[i] = false;
      if (k < deg) {
        const Ent e = load_ent(g, row, k);
        c4[i] = mp_match(req, et[k]);
        if (c4[i]) d = (double)e.w / S;
      }
      run += d;
      l[i] = run;
    }
    const double incl = wave_incl_scan_f64(run);
    double excl = __shfl_up(incl, 1);                   // pure additions only: no (incl - run) cancellation
    if (lane == 0) excl = 0.0;
    const double lane_base = carry + excl;
    int firsti = 4;          // first of my 4 entries that is a candidate and not a certain miss
    bool sure = false;
#pragma unroll
    for (int i = 3; i >= 0; --i) {
      const double acc = lane_base + l[i];
      const double tol = (double)(k0 + i + 1) * 0x1p-51 * acc;
      if (c4[i] && !(acc + tol < p)) { firsti = i; sure = (acc - tol >= p); }
    }
    const unsigned long long open = __ballot(firsti < 4);
    if (open) {
      const int fl = __ffsll((long long)open) - 1;
      const int fi = __builtin_amdgcn_readlane(firsti, fl);
      if (__builtin_amdgcn_readlane((int)sure, fl)) return base + fl * 4 + fi;
      fallback = 1;                                      // within rounding distance of a boundary: exact chain
      return wave_chain_pick_typed(g, row, et, deg, req, p, S, head);
    }
    carry += readlane_f64(incl, 63);
  }
  return head;                                           // every candidate a certain miss: the sublist's head (:24)
}

__global__ __launch_bounds__(TPB, 4) void k_walk_metapath(GraphView g, const int32_t *__restrict__ verts, int64_t n_verts, int64_t n_walkers,
                                                          int32_t L, int32_t first_walk, RngSpec rng, MetaPattern pat,
                                                          const uint8_t *__restrict__ etype, const uint8_t *__restrict__ vtypes,
                                                          const int32_t *__restrict__ vpos, int32_t *__restrict__ paths,
                                                          int32_t *__restrict__ lens, DevCounters *ctr, unsigned long long *cursor) {
  const int lane = lane_id();
  const int64_t stride = (int64_t)L + 2;
  unsigned long long steps = 0, dead = 0, fb = 0;
  while (true) {                                         // persistent waves: the next walker from the cursor (k_walk_general)
    unsigned long long grab = 0;
    if (lane == 0) grab = atomicAdd(cursor, 1ull);
    const int64_t wi = (int64_t)(((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(grab >> 32)) << 32) |
                                 (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)grab));
    if (wi >= n_walkers) break;
    const int64_t it = wi / n_verts, vi = wi - it * n_verts;
    const uint32_t iter = (uint32_t)(first_walk + it);
    const int32_t src = verts[vi];
    const uint32_t ksrc = (uint32_t)rng_source(g, src);   // Philox key: the input's id of the source
    int32_t *path = paths + wi * stride;
    if (lane == 0) path[0] = src;
    int32_t curr = src, len = 1;
    // position 0: the source's own type
    bool go = true;
    {
      const int req0 = pat.t[0];
      if (req0 >= 0) {
        const int64_t ss = (int64_t)src - g.vmin;
        const int32_t vp = (ss >= 0 && ss < g.n_slots) ? vpos[ss] : -1;
        go = vp >= 0 && (int)vtypes[vp] == req0;
      }
    }
    int32_t j = pat.m > 1 ? 1 : 0;                       // s mod m, kept by increments
    for (int32_t s = 1; go && s <= L + 1; ++s) {
      const int64_t cslot = (int64_t)curr - g.vmin;
      const bool in_range = cslot >= 0 && cslot < g.n_slots;
      Row r = g.rows[in_range ? cslot : 0];
      if (!in_range) { r.off = 0; r.deg = 0; r.flags = 0; }
      r = uniform_row(r);
      if (r.deg == 0) { dead += s > 1; break; }
      const int req = pat.t[j];
      const float u = draw_uniform(rng, iter, ksrc, (uint32_t)s);
      unsigned f = 0;
      const int32_t k = wave_pick_typed(g, r, etype, req, u, f);
      if (k < 0) { dead += s > 1; break; }               // no neighbor of the step's type: the walk ends
      fb += f;
      const int32_t next = load_ent(g, g.ent + r.off, k).id;
      if (lane == 0) path[s] = next;
      curr = next; ++len;
      j = j + 1 == pat.m ? 0 : j + 1;
    }
    for (int64_t t = len + lane; t < stride; t += 64) path[t] = -1;  // unused tail
    if (lane == 0) lens[wi] = len;
    steps += (unsigned long long)(len - 1);
  }
  if (lane == 0) {
    if (steps) atomicAdd(&ctr->steps, steps);
    if (dead) atomicAdd(&ctr->dead_ends, dead);
    if (fb) atomicAdd(&ctr->fallbacks, fb);
  }
}

}  // namespace

void vertex_types_clear(srw_handle *h) {
  h->g.vtypes.release(); h->g.etype.release(); h->g.has_types = false;
}

void vertex_types_set(srw_handle *h, const uint8_t *d_types, int64_t n) {
  Graph &g = h->g;
  hipStream_t st = h->stream;
  DevBuf<uint8_t> vt, et;                                // an allocation that fails leaves the types in force as they are
  vt.alloc((size_t)n);
  et.alloc((size_t)g.n_entries);
  if (n > 0) SRW_HIP(hipMemcpyAsync(vt.p, d_types, (size_t)n, hipMemcpyDeviceToDevice, st));
  ensure_vpos(h);
  if (g.n_entries > 0) {
    const int64_t nb = std::min<int64_t>((g.n_entries + TPB - 1) / TPB, (int64_t)h->n_cus * 16);
    hipLaunchKernelGGL(k_entry_types, dim3((unsigned)nb), dim3(TPB), 0, st, (const Ent *)g.ent.p, g.n_entries, (const Row *)g.rows.p, g.n_slots,
                       g.vmin, (const int32_t *)g.vpos.p, (const uint8_t *)vt.p, et.p);
    SRW_HIP(hipGetLastError());
  }
  SRW_HIP(hipStreamSynchronize(st));
  g.vtypes = std::move(vt); g.etype = std::move(et); g.has_types = true;
}

void run_walk_metapath(srw_handle *h, const srw_walk_params &P, const int32_t *pattern, int32_t m, srw_walk_stats *stats) {
  Graph &g = h->g;
  auto refuse = [](const std::string &why) { throw Error(SRW_ERR_INVALID, "srw_walk_metapath: " + why); };
  if (!g.loaded) refuse("no graph loaded");
  if (h->cfg.world != 1) refuse("needs a whole-graph handle (world == 1)");
  if (!g.has_types) refuse("no vertex types in force (srw_vertex_types_set)");
  if (m < 1 || m > MP_MAX) refuse("m = " + std::to_string(m) + " is outside 1 .. 64");
  MetaPattern pat;
  memset(&pat, 0, sizeof(pat));
  pat.m = m;
  for (int32_t i = 0; i < m; ++i) {
    if (pattern[i] < -1 || pattern[i] > 255) refuse("pattern[" + std::to_string(i) + "] = " + std::to_string(pattern[i]) + " is outside -1 .. 255");
    pat.t[i] = (int16_t)pattern[i];
  }
  if (P.p != 1.0f || P.q != 1.0f) refuse("a typed step is first-order: p and q must both be 1");
  if (P.sampler != SRW_SAMPLER_REFERENCE) refuse("sampler must be SRW_SAMPLER_REFERENCE");
  check_params(P);                                       // walk_length, num_walks, rng_mode: what srw_walk refuses
  hipStream_t st = h->stream;
  const int32_t *verts = h->start_verts();
  const int64_t n_verts = h->walkers_per_iteration();
  const int64_t n_walkers = (int64_t)P.num_walks * n_verts;
  if (n_walkers >= ((int64_t)1 << 31)) refuse("more than 2^31 walkers in one call: lower num_walks");
  const int32_t stride = P.walk_length + 2;
  srw_walk_stats local;
  srw_walk_stats *s = stats ? stats : &local;
  if (n_walkers == 0) {   // empty graph, empty source list or num_walks == 0: nothing to walk
    h->res.n_walkers = 0; h->res.stride = stride; h->res.valid = true;
    memset(s, 0, sizeof(*s)); s->kernel_kind = 4;
    return;
  }
  ensure_vpos(h);                                        // (the source's type; built with the types, rebuilt if something dropped it)
  h->res.valid = false;
  h->res.paths.ensure((size_t)n_walkers * stride);
  h->res.lens.ensure((size_t)n_walkers);
  h->res.n_walkers = n_walkers; h->res.stride = stride;
  h->counters.ensure(1);
  h->walk_cursor.ensure(2);
  SRW_HIP(hipMemsetAsync(h->counters.p, 0, sizeof(DevCounters), st));
  SRW_HIP(hipMemsetAsync(h->walk_cursor.p, 0, 2 * sizeof(unsigned long long), st));
  RngSpec rng; rng.mode = P.rng_mode; rng.const_r = P.const_r; rng.seed = P.seed;
  SRW_HIP(hipEventRecord(h->ev0, st));
  const int64_t blocks = std::min<int64_t>((n_walkers * 64 + TPB - 1) / TPB, (int64_t)h->n_cus * 8);
  hipLaunchKernelGGL(k_walk_metapath, dim3((unsigned)blocks), dim3(TPB), 0, st, g.view(), verts, n_verts, n_walkers, P.walk_length, P.first_walk,
                     rng, pat, (const uint8_t *)g.etype.p, (const uint8_t *)g.vtypes.p, (const int32_t *)g.vpos.p, h->res.paths.p, h->res.lens.p,
                     h->counters.p, h->walk_cursor.p);
  SRW_HIP(hipGetLastError());
  // compacted ids: the kernel walked over ranks; the paths leave with the ids of the input
  if (g.compact) paths_to_ids(h, h->res.paths.p, h->res.lens.p, n_walkers, stride);
  SRW_HIP(hipEventRecord(h->ev1, st));
  DevCounters c;
  SRW_HIP(hipMemcpyAsync(&c, h->counters.p, sizeof(c), hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  SRW_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  memset(s, 0, sizeof(*s));
  s->n_walkers = n_walkers; s->n_steps = (int64_t)c.steps; s->dead_ends = (int64_t)c.dead_ends; s->fallbacks = (int64_t)c.fallbacks;
  s->kernel_ms = ms; s->kernel_kind = 4;
  h->res.valid = true;
}

}  // namespace srw
