// Top-k item retrieval over item embeddings: scores = Q . C^T (inner) or the cosine of the rows, and for
// every query the k best catalogue rows, without the [Nq][Nc] score matrix ever leaving the chip.
//
//  1. topk_norm_kernel    inverse row norms of Q (cosine; norms clamped at 1e-8 as align.hip's
//                         cosine_similarity) or 1.0 (inner): one wave per row, fixed summation order.  The
//                         catalogue's are summed inside the tile kernel from the rows it stages (RowSquares): a
//                         pass of their own would read the catalogue from HBM a second time.
//  2. topk_tile_kernel    a workgroup owns TQ queries and one CHUNK of the catalogue, which it streams in
//                         TC-row tiles through the exact-f32 MFMA main loop (gemm_f32_tile.h's) with the
//                         catalogue as the A (row) operand: a lane's 16 accumulators of a 32x32 tile are then
//                         16 catalogue rows of ONE query (column lane & 31), so the running top-k of that
//                         query over the rows this lane sees lives in the lane's own registers -- no LDS, no
//                         ownership between waves.  An entry is one 64-bit key
//                             (order-preserving bits of the score) << 32 | (0xffffffff - catalogue row)
//                         so "higher score, then lower index" is one unsigned compare; the list is kept sorted
//                         by a compare-exchange chain that runs only when some lane of the wave holds a score
//                         not below its list's k-th.  Each lane leaves its k keys in the workspace.
//  3. topk_merge_kernel   one workgroup per query merges the lane lists (2 x WM per chunk), and with
//                         `accumulate` the incoming (scores, idx), into the sorted output.
//
// Determinism: a score is the MFMA's k-ordered fmaf chain over the whole of H for its (query, row) pair, then
// (dot * 1/|q|) * 1/|c|: it does not depend on the tile, chunk or block that computed it.  (score, index) is a
// strict total order, so the k best of a set do not depend on how the set was split or in which order the parts
// were merged: any chunk count and any split into accumulate blocks give the same bits.  No atomics.
#include "gemm_f32_tile.h"

#include <climits>

namespace {

using namespace K3M_F32_NS;

constexpr int MAXK = 64;
constexpr int MERGE_NW = 16;   // waves of a merge workgroup

__device__ __forceinline__ uint32_t ord_bits(float s) {   // unsigned order == float order (no NaN)
  const uint32_t b = __float_as_uint(s);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float unord_bits(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? o ^ 0x80000000u : ~o);
}
__device__ __forceinline__ bool beats(float as, long long ai, float bs, long long bi) {
  return as > bs || (as == bs && ai < bi);
}

__global__ __launch_bounds__(256) void topk_norm_kernel(const float* __restrict__ x, int rows, int H, int cosine,
                                                        float* __restrict__ inv) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  float ss = 0.f;
  if (cosine) {
    const float* p = x + (long long)row * H;
    for (int c = 4 * lane; c < H; c += 256) {
      const floatx4 v = *reinterpret_cast<const floatx4*>(p + c);
      ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    ss = wave_sum(ss);
  }
  if (lane == 0) inv[row] = cosine ? 1.f / fmaxf(sqrtf(ss), 1e-8f) : 1.f;
}

// Sum of squares of the catalogue rows of a tile, taken from the main loop's staged registers (the data the tile
// loads anyway: no second pass over the catalogue).  Thread t stages the 16-B piece (t + NT it) & 7 of row
// (t + NT it) >> 3 in every k-tile: ss[it] sums that piece's squares over the k-tiles in k order, and the row's
// eight pieces sit on eight consecutive lanes (reduced by XOR shuffles).  The order is fixed and the same for every
// tile shape, so 1/|c| of a row does not depend on the tiling.
template <int TC, int NT>
struct RowSquares {
  static constexpr int NB = TC * 8 / NT;
  float ss[NB];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int it = 0; it < NB; ++it) ss[it] = 0.f;
  }
  __device__ __forceinline__ void operator()(const Stage<true, TC, NT>& s) {
#pragma unroll
    for (int it = 0; it < NB; ++it) {
      const floatx4 v = s.r[it];
      ss[it] = fmaf(v[3], v[3], fmaf(v[2], v[2], fmaf(v[1], v[1], fmaf(v[0], v[0], ss[it]))));
    }
  }
  // inv[row of the tile] = 1 / max(|c|, 1e-8) (cosine) or 1 (inner)
  __device__ __forceinline__ void finish(float* inv, bool cosine) {
#pragma unroll
    for (int it = 0; it < NB; ++it) {
      float v = ss[it];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      const int idx = threadIdx.x + NT * it;
      if ((idx & 7) == 0) inv[idx >> 3] = cosine ? 1.f / fmaxf(sqrtf(v), 1e-8f) : 1.f;
    }
  }
};

// gemm_f32_tile.h's main loop (both operands k-contiguous, 16-B vectors, the whole of K) with one addition: sq sees
// the thread's staged A registers of every k-tile, in k order.  The loop is restated here, over the header's staging
// and LDS image (load_tile / store_tile / swz: the operand layout and the k order stay the header's), because a hook
// parameter in the header's mainloop, even one that the GEMM kernels leave at a no-op default, changed the
// instruction schedule of every fp32 GEMM kernel.
template <int TC, int TQ, int WM, int WN>
__device__ __forceinline__ void mainloop_sq(const float* __restrict__ A, const float* __restrict__ B, int H, int M,
                                            int N, int m0, int n0, float* smem, floatx16 (&acc)[TC / WM / 32][1],
                                            RowSquares<TC, 64 * WM * WN>& sq) {
  constexpr int NT = 64 * WM * WN, FM = TC / WM / 32, BUF = (TC + TQ) * BK;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wm = (w / WN) * (TC / WM), wn = (w % WN) * 32;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;
  Stage<true, TC, NT> ra;
  Stage<true, TQ, NT> rb;
  const int nk = (H + BK - 1) / BK;
  load_tile<true, true, TC, NT>(A, H, m0, 0, M, H, ra);
  load_tile<true, true, TQ, NT>(B, H, n0, 0, N, H, rb);
  store_tile<true, TC, NT>(smem, ra);
  store_tile<true, TQ, NT>(smem + TC * BK, rb);
  sq(ra);
  __syncthreads();
  const int h = lane >> 5, cl = lane & 31;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) {
      load_tile<true, true, TC, NT>(A, H, m0, (kt + 1) * BK, M, H, ra);
      load_tile<true, true, TQ, NT>(B, H, n0, (kt + 1) * BK, N, H, rb);
    }
    const float* as = smem + cur * BUF;
    const float* bs = as + TC * BK;
#pragma unroll
    for (int j4 = 0; j4 < 4; ++j4) {
      floatx4 a[FM];
#pragma unroll
      for (int i = 0; i < FM; ++i) a[i] = *reinterpret_cast<const floatx4*>(as + swz(wm + 32 * i + cl, 4 * h + j4));
      const floatx4 b = *reinterpret_cast<const floatx4*>(bs + swz(wn + cl, 4 * h + j4));
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < FM; ++i)
          acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][q], b[q], acc[i][0], 0, 0, 0);
    }
    if (more) {
      store_tile<true, TC, NT>(smem + (cur ^ 1) * BUF, ra);
      store_tile<true, TQ, NT>(smem + (cur ^ 1) * BUF + TC * BK, rb);
      sq(ra);
    }
    __syncthreads();
  }
}

// part: [nlists][Nq][k] keys, list = (chunk * WM + wave row) * 2 + lane half; 0 = empty slot.
template <int TC, int TQ, int WM, int WN, int KP>
__global__ __launch_bounds__(64 * WM * WN, 1) void topk_tile_kernel(
    const float* __restrict__ Q, const float* __restrict__ Cm, int Nq, int Nc, int H, int k,
    const float* __restrict__ qinv, int cosine, const long long* __restrict__ q_ids,
    long long c_base, int tiles, int tiles_per_chunk, int qtiles, unsigned long long* __restrict__ part) {
  static_assert(TQ == 32 * WN, "one 32-query MFMA column block per wave");
  constexpr int FM = TC / WM / 32;
  __shared__ __attribute__((aligned(16))) float smem[2 * (TC + TQ) * BK];
  __shared__ __attribute__((aligned(16))) float cinv[TC];   // 1/|c| of the tile's rows
  RowSquares<TC, 64 * WM * WN> sq;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int chunk = id / qtiles, n0 = (id % qtiles) * TQ;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5;
  const int wmi = w / WN, wm = wmi * (TC / WM), wn = (w % WN) * 32;
  const int q = n0 + wn + (lane & 31);
  const bool qvalid = q < Nq;
  const float qi = qvalid ? qinv[q] : 0.f;
  int excl = -1;   // the catalogue row this query must not retrieve
  if (q_ids && qvalid) {
    const long long qid = q_ids[q];
    if (qid != -1 && qid >= c_base && qid - c_base < (long long)Nc) excl = (int)(qid - c_base);
  }

  unsigned long long L[KP];
#pragma unroll
  for (int p = 0; p < KP; ++p) L[p] = 0ull;
  float thr_f = -INFINITY;   // score of the list's k-th entry

  const int t1 = min(tiles, (chunk + 1) * tiles_per_chunk);
  for (int t = chunk * tiles_per_chunk; t < t1; ++t) {
    const int m0 = t * TC;
    floatx16 acc[FM][1];
    sq.clear();
    mainloop_sq<TC, TQ, WM, WN>(Cm, Q, H, Nc, Nq, m0, n0, smem, acc, sq);
    // (the main loop ended on a barrier, and every wave has passed one since it last read cinv)
    sq.finish(cinv, cosine != 0);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int base = m0 + wm + 32 * i + 4 * h;   // + (r & 3) + 8 (r >> 2): the row of accumulator r
      floatx4 ci[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) ci[g] = *reinterpret_cast<const floatx4*>(cinv + (base - m0) + 8 * g);
      float sc[16];
      uint32_t cm = 0u;   // bit r: accumulator r is a candidate
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = base + (r & 3) + 8 * (r >> 2);
        sc[r] = (acc[i][0][r] * qi) * ci[r >> 2][r & 3] + 0.f;   // + 0: -0 -> +0, one key per value
        cm |= (uint32_t)(sc[r] >= thr_f && row < Nc && row != excl) << r;
      }
      if (!qvalid) cm = 0u;
      while (__ballot(cm != 0u)) {
        // every lane takes its lowest candidate; lanes without one carry the empty key through the chain
        const int r = cm ? __builtin_ctz(cm) : 16;
        cm &= cm - 1u;
        float s = 0.f;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) s = r == rr ? sc[rr] : s;
        const uint32_t row = (uint32_t)(base + (r & 3) + 8 * (r >> 2));
        unsigned long long key = r < 16 ? ((unsigned long long)ord_bits(s) << 32) | (0xffffffffu - row) : 0ull;
        unsigned long long kth = 0ull;
#pragma unroll
        for (int p = 0; p < KP; ++p) {
          if (p < k) {   // wave-uniform
            const bool gt = key > L[p];
            const unsigned long long old = L[p];
            L[p] = gt ? key : old;
            key = gt ? old : key;
            if (p == k - 1) kth = L[p];
          }
        }
        thr_f = kth ? unord_bits((uint32_t)(kth >> 32)) : -INFINITY;
      }
    }
  }
  if (qvalid) {
    const int list = (chunk * WM + wmi) * 2 + h;
    unsigned long long* o = part + ((long long)list * Nq + q) * k;
#pragma unroll
    for (int p = 0; p < KP; ++p)
      if (p < k) o[p] = L[p];
  }
}

// One workgroup per query: wave w folds lists w, w + MERGE_NW, ... into a sorted list held one entry per lane
// (lane p = rank p), the waves' lists meet in LDS and wave 0 folds them, and the incoming result, the same way.
__global__ __launch_bounds__(64 * MERGE_NW) void topk_merge_kernel(const unsigned long long* __restrict__ part,
                                                                    int nlists, int Nq, int k, long long c_base,
                                                                    int accumulate, float* __restrict__ scores,
                                                                    long long* __restrict__ idx) {
  __shared__ float ls[MERGE_NW][MAXK];
  __shared__ long long li[MERGE_NW][MAXK];
  const int q = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float ms = -INFINITY;       // this lane's entry of the running list; (-inf, LLONG_MAX) = empty
  long long mi = LLONG_MAX;
  // a sorted candidate list, entry t on lane t: entries are inserted until one no longer beats the k-th
  auto fold = [&](float cs_l, long long ci_l) {
    for (int t = 0; t < k; ++t) {
      const float cs = __shfl(cs_l, t, 64);
      const long long cidx = __shfl(ci_l, t, 64);
      if (!beats(cs, cidx, __shfl(ms, k - 1, 64), __shfl(mi, k - 1, 64))) break;
      const bool b = beats(cs, cidx, ms, mi);
      const bool pb = __shfl_up((int)b, 1, 64) != 0 && lane > 0;
      const float ps = __shfl_up(ms, 1, 64);
      const long long pi = __shfl_up(mi, 1, 64);
      if (b) {
        ms = pb ? ps : cs;
        mi = pb ? pi : cidx;
      }
    }
  };
  constexpr int AHEAD = 8;   // lists loaded before the first of them is folded (a fold per load exposed every latency)
  for (int l0 = w; l0 < nlists; l0 += MERGE_NW * AHEAD) {
    unsigned long long key[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const int l = l0 + u * MERGE_NW;
      key[u] = (l < nlists && lane < k) ? part[((long long)l * Nq + q) * k + lane] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const float cs_l = key[u] ? unord_bits((uint32_t)(key[u] >> 32)) : -INFINITY;
      const long long ci_l = key[u] ? c_base + (long long)(0xffffffffu - (uint32_t)key[u]) : LLONG_MAX;
      fold(cs_l, ci_l);
    }
  }
  ls[w][lane] = ms;
  li[w][lane] = mi;
  __syncthreads();
  if (w != 0) return;
  for (int o = 1; o < MERGE_NW; ++o) fold(ls[o][lane], li[o][lane]);
  if (accumulate) {
    float cs_l = -INFINITY;
    long long ci_l = LLONG_MAX;
    if (lane < k) {
      cs_l = scores[(long long)q * k + lane];
      ci_l = idx[(long long)q * k + lane];
      if (ci_l < 0) {   // a padding slot of the earlier result
        cs_l = -INFINITY;
        ci_l = LLONG_MAX;
      }
    }
    fold(cs_l, ci_l);
  }
  if (lane < k) {
    const bool none = mi == LLONG_MAX;
    scores[(long long)q * k + lane] = none ? -INFINITY : ms;
    idx[(long long)q * k + lane] = none ? -1ll : mi;
  }
}

// Tiling of one call.  Many queries: 128 x 128 tiles, four waves side by side on the queries.  Up to 64 queries:
// 256 catalogue rows x 64 queries, 2 x 2 waves, so that the MFMAs are not spent on absent queries.
struct Plan {
  int small, tc, tq, wm, qtiles, tiles, chunks, tiles_per_chunk, nlists;
  long long off_part, bytes;
};

constexpr int NUM_CU = 256;
constexpr int MAX_CHUNKS = 1024;

Plan make_plan(int nq, int nc, int k, int chunks) {
  Plan p;
  p.small = nq <= 64;
  p.tc = p.small ? 256 : 128;
  p.tq = p.small ? 64 : 128;
  p.wm = p.small ? 2 : 1;
  p.qtiles = k3m_cdiv(nq, p.tq);
  p.tiles = k3m_cdiv(nc, p.tc);
  if (chunks <= 0) chunks = k3m_cdiv(NUM_CU, p.qtiles > 0 ? p.qtiles : 1);   // one workgroup per CU or more
  chunks = chunks > MAX_CHUNKS ? MAX_CHUNKS : chunks;
  chunks = chunks > p.tiles ? p.tiles : chunks;
  p.tiles_per_chunk = chunks > 0 ? k3m_cdiv(p.tiles, chunks) : 0;
  p.chunks = chunks > 0 ? k3m_cdiv(p.tiles, p.tiles_per_chunk) : 0;   // no empty chunk
  p.nlists = p.chunks * p.wm * 2;
  const long long nqp = ((long long)nq + 3) / 4 * 4;
  p.off_part = nqp * 4;   // after 1/|q|
  p.bytes = p.off_part + (long long)p.nlists * nq * k * 8;
  return p;
}

template <int TC, int TQ, int WM, int WN>
int launch_tiles(const Plan& p, const float* q, const float* c, int nq, int nc, int h, int k, const float* qinv,
                 int cosine, const long long* q_ids, long long c_base, unsigned long long* part, hipStream_t st) {
  const dim3 grid(p.qtiles * p.chunks), block(64 * WM * WN);
#define K3M_TOPK_LAUNCH(KP)                                                                                        \
  hipLaunchKernelGGL((topk_tile_kernel<TC, TQ, WM, WN, KP>), grid, block, 0, st, q, c, nq, nc, h, k, qinv, cosine, \
                     q_ids, c_base, p.tiles, p.tiles_per_chunk, p.qtiles, part)
  if (k <= 16) K3M_TOPK_LAUNCH(16);
  else if (k <= 32) K3M_TOPK_LAUNCH(32);
  else K3M_TOPK_LAUNCH(64);
#undef K3M_TOPK_LAUNCH
  K3M_CHECK_LAUNCH();
  return 0;
}

bool topk_args_ok(int nq, int nc, int h, int k, int chunks) {
  return nq >= 0 && nc >= 0 && k >= 1 && k <= MAXK && h >= 4 && h <= 4096 && h % 4 == 0 && chunks >= 0;
}

}  // namespace

extern "C" int k3m_topk_sim_ws_bytes(int nq, int nc, int h, int k, int chunks, long long* bytes) {
  K3M_ARG(bytes && topk_args_ok(nq, nc, h, k, chunks));
  *bytes = make_plan(nq, nc, k, chunks).bytes;
  return 0;
}

extern "C" int k3m_topk_sim(const float* q, const float* c, int nq, int nc, int h, int k, int metric,
                            long long c_base, const long long* q_ids, int accumulate, int chunks, float* scores,
                            long long* idx, void* ws, long long ws_bytes, hipStream_t st) {
  K3M_ARG(topk_args_ok(nq, nc, h, k, chunks) && (metric == K3M_TOPK_INNER || metric == K3M_TOPK_COSINE));
  if (nq == 0) return 0;
  K3M_ARG(q && scores && idx && (c || nc == 0));
  K3M_ARG(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0);
  const Plan p = make_plan(nq, nc, k, chunks);
  K3M_ARG(ws && ws_bytes >= p.bytes);
  char* wsb = static_cast<char*>(ws);
  float* qinv = reinterpret_cast<float*>(wsb);
  unsigned long long* part = reinterpret_cast<unsigned long long*>(wsb + p.off_part);
  if (nc > 0) {
    const int cosine = metric == K3M_TOPK_COSINE;
    hipLaunchKernelGGL(topk_norm_kernel, dim3(k3m_cdiv(nq, 4)), dim3(256), 0, st, q, nq, h, cosine, qinv);
    K3M_CHECK_LAUNCH();
    const int rc = p.small ? launch_tiles<256, 64, 2, 2>(p, q, c, nq, nc, h, k, qinv, cosine, q_ids, c_base, part, st)
                           : launch_tiles<128, 128, 1, 4>(p, q, c, nq, nc, h, k, qinv, cosine, q_ids, c_base, part, st);
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(topk_merge_kernel, dim3(nq), dim3(64 * MERGE_NW), 0, st, part, p.nlists, nq, k, c_base,
                     accumulate, scores, idx);
  K3M_CHECK_LAUNCH();
  return 0;
}
