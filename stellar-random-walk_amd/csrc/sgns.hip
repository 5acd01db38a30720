// sgns.hip — srw_sgns_step: one skip-gram negative-sampling step over the pos [W][C] / neg [W][K] tensors srw_skipgram_windows and
// srw_skipgram_batch write, on the caller's two float32 tables [nV][D].  Semantics: include/stellar_rw.h, DESIGN §7e.
//
//   k_vpos        vpos[slot] = position of the slot's vertex in V (the ascending list of present vertices), -1 for a slot that is no
//                 present vertex: the tables' rows are indexed by position in V, the ids resolve to slots.  Built once per graph.
//   k_sgns_step   ONE WAVE PER WINDOW, grid-stride over the windows, lanes across the vector: lane l holds elements l, l + 64, ... of a
//                 row (ND = D / 64 floats per lane), so every load and every atomic wave-instruction covers 256 contiguous bytes of one
//                 row — the shape global float atomics run at full rate in; one lane per row is 17 times slower.
//                 The window's C + K ids are resolved once, one id per lane (vertex_slot, device_common.h: what k_vertex_count
//                 resolves with), and checked (< nV) in that lane; one ballot decides whether the window is skipped whole; only then
//                 are positions broadcast (v_readlane) and turned into addresses.  The centre row and the running sum of
//                 g_i out[t_i] stay in registers over the window's targets; the targets go four at a time — all reads are of the OLD
//                 tables, so they are independent: four rows loaded, four dot products in one reduction (wave_sum4_f32), f -> g and
//                 the loss term once, in the lanes that hold the sums, then four rows of no-return float atomics into out_new and,
//                 after the last group, one row into in_new.  A target whose g is exactly 0 (lr == 0) adds nothing and is not written.
//                 No LDS, no scratch: 2 ND + 4 ND floats per lane at most (48 at D = 512).
//
// Exact and in-place (Hogwild) forms are the same kernel: in_new / out_new are separate buffers, or the old tables themselves.
#include <cmath>

#include "engine.h"
#include "wave_primitives.h"

namespace srw {
namespace {
constexpr int SG_TPB = 256;
constexpr int SG_BLOCKS_PER_CU = 8;
constexpr int SG_G = 4;                 // targets per reduction

__global__ __launch_bounds__(SG_TPB) void k_vpos(const int32_t *__restrict__ verts, int64_t nV, int32_t vmin, int32_t *__restrict__ vpos) {
  const int64_t i = (int64_t)blockIdx.x * SG_TPB + threadIdx.x;
  if (i < nV) vpos[(int64_t)verts[i] - vmin] = (int32_t)i;      // (verts[] holds slot + vmin: graph_build.hip:k_scatter_verts)
}

struct SgnsArgs {
  const int32_t *pos, *neg;             // [W][C], [W][K]
  int64_t W;
  int32_t C, K, center;
  float lr;
  const float *in, *out;                // the old tables [nV][64 ND]
  float *in_new, *out_new;              // where the adds go (the old tables themselves: in place)
  float *loss;                          // [W] or nullptr
  unsigned long long *skipped;          // windows that hold an id which is no present vertex
  const Row *rows; const int32_t *orig_id; const int32_t *vpos;
  int64_t n_slots; int32_t vmin; int32_t nV;
};

// softplus(x) = log(1 + e^x), finite for every finite x
__device__ inline float softplus_f32(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
// sigma(x) without an overflowing intermediate: e = e^-|x| <= 1
__device__ inline float sigmoid_f32(float x) {
  const float e = expf(-fabsf(x));
  return (x >= 0.0f ? 1.0f : e) / (1.0f + e);
}

template <int ND>
__global__ __launch_bounds__(SG_TPB) void k_sgns_step(const SgnsArgs a) {
  constexpr int64_t D = 64 * ND;
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * (SG_TPB / 64) + (int64_t)uni((int32_t)(threadIdx.x >> 6));
  const int64_t n_waves = (int64_t)gridDim.x * (SG_TPB / 64);
  const int32_t C = a.C, K = a.K, n_ids = C + K, T = n_ids - 1, center = a.center;
  unsigned long long n_skip = 0;
  for (int64_t w = wave; w < a.W; w += n_waves) {
    // lane l < C: pos[w][l]; C <= l < C + K: neg[w][l - C] -> its position in V, -1 when it has none
    int32_t p = -1;
    if (lane < n_ids) {
      const int32_t id = lane < C ? a.pos[w * C + lane] : a.neg[w * K + (lane - C)];
      const int64_t s = vertex_slot(id, a.rows, a.orig_id, a.n_slots, a.vmin);
      if (s < a.n_slots) p = a.vpos[s];
      if ((uint32_t)p >= (uint32_t)a.nV) p = -1;       // nothing that is not < nV leaves this lane as a position
    }
    if (__ballot(lane < n_ids && p < 0)) {             // skipped whole: no add, loss 0
      ++n_skip;
      if (a.loss && lane == 0) a.loss[w] = 0.0f;
      continue;
    }
    const int64_t c = (int64_t)__builtin_amdgcn_readlane(p, center);
    float vc[ND], acc[ND];
    {
      const float *rc = a.in + c * D + lane;
#pragma unroll
      for (int i = 0; i < ND; ++i) { vc[i] = rc[64 * i]; acc[i] = 0.0f; }
    }
    float loss = 0.0f;
    bool moved = false;                                // some g of this window is not 0
    for (int32_t t0 = 0; t0 < T; t0 += SG_G) {
      // target i is lane i of the id register below the centre, lane i + 1 from it on; a slot past the last target reads the centre's
      // row (a row that exists) and gets g = 0
      int64_t tp[SG_G];
      float vt[SG_G][ND], part[SG_G];
#pragma unroll
      for (int u = 0; u < SG_G; ++u) {
        const int32_t i = t0 + u;
        tp[u] = i < T ? (int64_t)__builtin_amdgcn_readlane(p, i < center ? i : i + 1) : c;
        const float *rt = a.out + tp[u] * D + lane;
#pragma unroll
        for (int k = 0; k < ND; ++k) vt[u][k] = rt[64 * k];
      }
#pragma unroll
      for (int u = 0; u < SG_G; ++u) {
        part[u] = 0.0f;
#pragma unroll
        for (int k = 0; k < ND; ++k) part[u] += vc[k] * vt[u][k];
      }
      // lanes 12 .. 15 of every row hold f of target t0 + (lane & 3): g and the loss term once, there, for all four
      const float f = wave_sum4_f32(part[0], part[1], part[2], part[3], lane);
      const int32_t il = t0 + (lane & 3);
      const bool positive = il < C - 1;
      const float sg = sigmoid_f32(positive ? -f : f);  // label - sigma(f) = sigma(-f) for label 1, -sigma(f) for label 0: no cancellation
      const float gl = il < T ? a.lr * (positive ? sg : -sg) : 0.0f;
      const float ll = il < T ? softplus_f32(positive ? -f : f) : 0.0f;
      float g[SG_G];
#pragma unroll
      for (int u = 0; u < SG_G; ++u) {
        g[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gl), 12 + u));
        loss += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ll), 12 + u));
      }
#pragma unroll
      for (int u = 0; u < SG_G; ++u) {
        if (g[u] != 0.0f) {                            // (wave-uniform; also false for the slots past the last target)
          moved = true;
          float *dst = a.out_new + tp[u] * D + lane;
#pragma unroll
          for (int k = 0; k < ND; ++k) {
            acc[k] += g[u] * vt[u][k];
            atomicAdd(dst + 64 * k, g[u] * vc[k]);
          }
        }
      }
    }
    if (moved) {
      float *dst = a.in_new + c * D + lane;
#pragma unroll
      for (int k = 0; k < ND; ++k) atomicAdd(dst + 64 * k, acc[k]);
    }
    if (a.loss && lane == 0) a.loss[w] = loss;
  }
  if (n_skip && lane == 0) atomicAdd(a.skipped, n_skip);
}

template <int ND>
void launch_sgns(srw_handle *h, const SgnsArgs &a) {
  const int64_t want = (a.W + SG_TPB / 64 - 1) / (SG_TPB / 64);
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)h->n_cus * SG_BLOCKS_PER_CU));
  hipLaunchKernelGGL(k_sgns_step<ND>, dim3(blocks), dim3(SG_TPB), 0, h->stream, a);
  SRW_HIP(hipGetLastError());
}
}  // namespace

// slot -> position in V, once per graph (a load drops it with the graph)
void ensure_vpos(srw_handle *h) {
  Graph &g = h->g;
  if (g.has_vpos) return;
  g.vpos.alloc((size_t)g.n_slots);
  SRW_HIP(hipMemsetAsync(g.vpos.p, 0xFF, (size_t)g.n_slots * 4, h->stream));
  if (g.n_vertices > 0) {
    hipLaunchKernelGGL(k_vpos, dim3((unsigned)((g.n_vertices + SG_TPB - 1) / SG_TPB)), dim3(SG_TPB), 0, h->stream,
                       (const int32_t *)g.verts.p, g.n_vertices, g.vmin, g.vpos.p);
    SRW_HIP(hipGetLastError());
  }
  g.has_vpos = true;
}

int64_t sgns_step(srw_handle *h, const int32_t *d_pos, const int32_t *d_neg, int64_t n_windows, const srw_sgns_params &sp,
                  const float *d_in, const float *d_out, float *d_in_new, float *d_out_new, float *d_loss) {
  const Graph &g = h->g;
  hipStream_t st = h->stream;
  ensure_vpos(h);
  h->sgns_skipped.ensure(1);
  SRW_HIP(hipMemsetAsync(h->sgns_skipped.p, 0, 8, st));
  SgnsArgs a{};
  a.pos = d_pos; a.neg = d_neg; a.W = n_windows;
  a.C = sp.context; a.K = sp.num_negatives; a.center = sp.center; a.lr = sp.lr;
  a.in = d_in; a.out = d_out; a.in_new = d_in_new; a.out_new = d_out_new; a.loss = d_loss;
  a.skipped = h->sgns_skipped.p;
  a.rows = g.rows.p; a.orig_id = g.compact ? g.orig_id.p : nullptr; a.vpos = g.vpos.p;
  a.n_slots = g.n_slots; a.vmin = g.vmin; a.nV = (int32_t)g.n_vertices;
  switch (sp.dim / 64) {
    case 1: launch_sgns<1>(h, a); break;
    case 2: launch_sgns<2>(h, a); break;
    case 3: launch_sgns<3>(h, a); break;
    case 4: launch_sgns<4>(h, a); break;
    case 5: launch_sgns<5>(h, a); break;
    case 6: launch_sgns<6>(h, a); break;
    case 7: launch_sgns<7>(h, a); break;
    default: launch_sgns<8>(h, a); break;
  }
  unsigned long long skipped = 0;
  SRW_HIP(hipMemcpyAsync(&skipped, h->sgns_skipped.p, 8, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  return (int64_t)skipped;
}

}  // namespace srw
