// Masked-position prediction: for every row of x [n][h] the k largest logits x . w[j] + bias[j] over a decoder
// w [v][h], the log-sum-exp of ALL v logits and the logit of one gold row, without the [n][v] logits ever leaving
// the chip.  The vocabulary-side sibling of topk.hip, whose design it takes:
//
//  1. topk_logits_tile_kernel   a workgroup owns TQ queries and one CHUNK of the vocabulary, which it streams in
//                               TC-row tiles through gemm_f32_tile.h's exact-f32 MFMA main loop with the decoder as
//                               the A (row) operand: a lane's 16 accumulators of a 32x32 tile are 16 vocabulary rows
//                               of ONE query (column lane & 31).  The tile's bias values are loaded before the main
//                               loop and staged in LDS once per tile.  Per lane, in registers:
//                                 * the running top-k of the rows this lane sees, one 64-bit key per entry
//                                       (order-preserving bits of the score) << 32 | (0xffffffff - row)
//                                   kept sorted by a compare-exchange chain that runs only when some lane of the
//                                   wave holds a score not below its list's k-th;
//                                 * an online (max, sum of exp(score - max)) pair over EVERY valid row;
//                               and the one lane of the whole grid that sees row == gold[query] stores that score.
//  2. topk_logits_merge_kernel  one workgroup per query merges the lane lists (2 x WM per chunk) into the sorted
//                               output and folds the (max, sum) pairs, in list order, into lse.
//
// Determinism: score = dot + bias[row] + 0, where dot is the MFMA's k-ordered fmaf chain over the whole of h for
// its (query, row) pair: its bits do not depend on tile, tiling or chunk, and (score, row) is a strict total order,
// so scores, idx and gold_score are bit-identical for every chunk count and both tilings.  lse sums in an order
// that the chunk count fixes: deterministic for a given `chunks`, summation rounding apart across them.  No atomics.
#include "gemm_f32_tile.h"

#include <climits>

namespace {

using namespace K3M_F32_NS;

constexpr int TL_MAXK = 32;
constexpr int TL_MERGE_NW = 16;   // waves of a merge workgroup

__device__ __forceinline__ uint32_t tl_ord_bits(float s) {   // unsigned order == float order (no NaN)
  const uint32_t b = __float_as_uint(s);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float tl_unord_bits(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? o ^ 0x80000000u : ~o);
}
__device__ __forceinline__ bool tl_beats(float as, long long ai, float bs, long long bi) {
  return as > bs || (as == bs && ai < bi);
}

// part: [nlists][n][k] keys, list = (chunk * WM + wave row) * 2 + lane half; 0 = empty slot.
// ms:   [nlists][n][2] the list's (max, sum of exp(score - max)); (-inf, 0) = no row seen.
template <int TC, int TQ, int WM, int WN, int KP>
__global__ __launch_bounds__(64 * WM * WN, 1) void topk_logits_tile_kernel(
    const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias, int n, int v, int H,
    int k, const long long* __restrict__ gold, int tiles, int tiles_per_chunk, int qtiles,
    unsigned long long* __restrict__ part, float* __restrict__ ms, float* __restrict__ gold_score) {
  static_assert(TQ == 32 * WN, "one 32-query MFMA column block per wave");
  static_assert(TC <= 64 * WM * WN, "one bias value per thread");
  constexpr int FM = TC / WM / 32;
  __shared__ __attribute__((aligned(16))) float smem[2 * (TC + TQ) * BK];
  __shared__ __attribute__((aligned(16))) float sbias[TC];   // bias of the tile's rows
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int chunk = id / qtiles, n0 = (id % qtiles) * TQ;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5;
  const int wmi = w / WN, wm = wmi * (TC / WM), wn = (w % WN) * 32;
  const int q = n0 + wn + (lane & 31);
  const bool qvalid = q < n;
  int grow = -1;   // the vocabulary row whose score this query reports
  if (gold_score && qvalid) {
    const long long g = gold[q];
    if (g >= 0 && g < (long long)v) grow = (int)g;
    else if (chunk == 0 && wmi == 0 && h == 0) gold_score[q] = -INFINITY;   // no lane will meet it
  }

  unsigned long long L[KP];
#pragma unroll
  for (int p = 0; p < KP; ++p) L[p] = 0ull;
  float thr_f = -INFINITY;   // score of the list's k-th entry
  float run_m = -INFINITY, run_s = 0.f;

  const int t1 = min(tiles, (chunk + 1) * tiles_per_chunk);
  for (int t = chunk * tiles_per_chunk; t < t1; ++t) {
    const int m0 = t * TC;
    float bv = 0.f;
    if (bias && (int)threadIdx.x < TC && m0 + (int)threadIdx.x < v) bv = bias[m0 + threadIdx.x];
    floatx16 acc[FM][1];
    mainloop<TC, TQ, WM, WN, true, true, true>(W, H, X, H, v, n, m0, n0, 0, H, smem, acc);
    // (the main loop ended on a barrier, and every wave has passed one since it last read sbias)
    if ((int)threadIdx.x < TC) sbias[threadIdx.x] = bv;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int base = m0 + wm + 32 * i + 4 * h;   // + (r & 3) + 8 (r >> 2): the row of accumulator r
      floatx4 bi[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) bi[g] = *reinterpret_cast<const floatx4*>(sbias + (base - m0) + 8 * g);
      float sc[16];
      uint32_t cm = 0u;   // bit r: accumulator r is a candidate
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = base + (r & 3) + 8 * (r >> 2);
        sc[r] = (acc[i][0][r] + bi[r >> 2][r & 3]) + 0.f;   // + 0: -0 -> +0, one key per value
        const bool rvalid = row < v;
        cm |= (uint32_t)(sc[r] >= thr_f && rvalid) << r;
        tmax = rvalid ? fmaxf(tmax, sc[r]) : tmax;
        if (row == grow) gold_score[q] = sc[r];   // grow >= 0 only on valid queries: one lane of the grid
      }
      if (qvalid && tmax > -INFINITY) {   // every valid row enters the log-sum-exp, candidate or not
        const float nm = fmaxf(run_m, tmax);
        float add = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = base + (r & 3) + 8 * (r >> 2);
          add += row < v ? __expf(sc[r] - nm) : 0.f;
        }
        run_s = run_s * __expf(run_m - nm) + add;   // run_m = -inf: run_s is 0 and exp gives 0
        run_m = nm;
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
        unsigned long long key = r < 16 ? ((unsigned long long)tl_ord_bits(s) << 32) | (0xffffffffu - row) : 0ull;
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
        thr_f = kth ? tl_unord_bits((uint32_t)(kth >> 32)) : -INFINITY;
      }
    }
  }
  if (qvalid) {
    const int list = (chunk * WM + wmi) * 2 + h;
    unsigned long long* o = part + ((long long)list * n + q) * k;
#pragma unroll
    for (int p = 0; p < KP; ++p)
      if (p < k) o[p] = L[p];
    float* mo = ms + ((long long)list * n + q) * 2;
    mo[0] = run_m;
    mo[1] = run_s;
  }
}

// One workgroup per query: wave w folds lists w, w + TL_MERGE_NW, ... into a sorted list held one entry per lane
// (lane p = rank p), the waves' lists meet in LDS and wave 0 folds them.  The last wave meanwhile folds the lists'
// (max, sum) pairs: lane l takes lists l, l + 64, ... in order, then a fixed XOR-shuffle tree over the lanes.
__global__ __launch_bounds__(64 * TL_MERGE_NW) void topk_logits_merge_kernel(
    const unsigned long long* __restrict__ part, const float* __restrict__ ms, int nlists, int n, int k,
    float* __restrict__ scores, long long* __restrict__ idx, float* __restrict__ lse) {
  __shared__ float ls[TL_MERGE_NW][TL_MAXK];
  __shared__ long long li[TL_MERGE_NW][TL_MAXK];
  const int q = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (w == TL_MERGE_NW - 1) {
    float m = -INFINITY;
    for (int l = lane; l < nlists; l += 64) m = fmaxf(m, ms[((long long)l * n + q) * 2]);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    float s = 0.f;
    for (int l = lane; l < nlists; l += 64) {
      const float lm = ms[((long long)l * n + q) * 2], lsum = ms[((long long)l * n + q) * 2 + 1];
      s += lm > -INFINITY ? lsum * __expf(lm - m) : 0.f;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) lse[q] = m > -INFINITY ? m + logf(s) : -INFINITY;
  }
  float msc = -INFINITY;      // this lane's entry of the running list; (-inf, LLONG_MAX) = empty
  long long mi = LLONG_MAX;
  // a sorted candidate list, entry t on lane t: entries are inserted until one no longer beats the k-th
  auto fold = [&](float cs_l, long long ci_l) {
    for (int t = 0; t < k; ++t) {
      const float cs = __shfl(cs_l, t, 64);
      const long long cidx = __shfl(ci_l, t, 64);
      if (!tl_beats(cs, cidx, __shfl(msc, k - 1, 64), __shfl(mi, k - 1, 64))) break;
      const bool b = tl_beats(cs, cidx, msc, mi);
      const bool pb = __shfl_up((int)b, 1, 64) != 0 && lane > 0;
      const float ps = __shfl_up(msc, 1, 64);
      const long long pi = __shfl_up(mi, 1, 64);
      if (b) {
        msc = pb ? ps : cs;
        mi = pb ? pi : cidx;
      }
    }
  };
  constexpr int AHEAD = 8;   // lists loaded before the first of them is folded
  for (int l0 = w; l0 < nlists; l0 += TL_MERGE_NW * AHEAD) {
    unsigned long long key[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const int l = l0 + u * TL_MERGE_NW;
      key[u] = (l < nlists && lane < k) ? part[((long long)l * n + q) * k + lane] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const float cs_l = key[u] ? tl_unord_bits((uint32_t)(key[u] >> 32)) : -INFINITY;
      const long long ci_l = key[u] ? (long long)(0xffffffffu - (uint32_t)key[u]) : LLONG_MAX;
      fold(cs_l, ci_l);
    }
  }
  if (lane < TL_MAXK) {
    ls[w][lane] = msc;
    li[w][lane] = mi;
  }
  __syncthreads();
  if (w != 0) return;
  for (int o = 1; o < TL_MERGE_NW; ++o) {
    const float cs_l = lane < TL_MAXK ? ls[o][lane] : -INFINITY;
    const long long ci_l = lane < TL_MAXK ? li[o][lane] : LLONG_MAX;
    fold(cs_l, ci_l);
  }
  if (lane < k) {
    const bool none = mi == LLONG_MAX;
    scores[(long long)q * k + lane] = none ? -INFINITY : msc;
    idx[(long long)q * k + lane] = none ? -1ll : mi;
  }
}

// Tiling of one call, as topk.hip's.  Many queries: 128 x 128 tiles, four waves side by side on the queries.  Up to
// 64 queries: 256 vocabulary rows x 64 queries, 2 x 2 waves, so that the MFMAs are not spent on absent queries.
struct TlPlan {
  int small, tc, tq, wm, qtiles, tiles, chunks, tiles_per_chunk, nlists;
  long long off_ms, bytes;
};

constexpr int TL_NUM_CU = 256;
constexpr int TL_MAX_CHUNKS = 1024;

TlPlan tl_plan(int n, int v, int k, int chunks) {
  TlPlan p;
  p.small = n <= 64;
  p.tc = p.small ? 256 : 128;
  p.tq = p.small ? 64 : 128;
  p.wm = p.small ? 2 : 1;
  p.qtiles = k3m_cdiv(n, p.tq);
  p.tiles = k3m_cdiv(v, p.tc);
  if (chunks <= 0) chunks = k3m_cdiv(TL_NUM_CU, p.qtiles > 0 ? p.qtiles : 1);   // one workgroup per CU or more
  chunks = chunks > TL_MAX_CHUNKS ? TL_MAX_CHUNKS : chunks;
  chunks = chunks > p.tiles ? p.tiles : chunks;
  p.tiles_per_chunk = chunks > 0 ? k3m_cdiv(p.tiles, chunks) : 0;
  p.chunks = chunks > 0 ? k3m_cdiv(p.tiles, p.tiles_per_chunk) : 0;   // no empty chunk
  p.nlists = p.chunks * p.wm * 2;
  p.off_ms = (long long)p.nlists * n * k * 8;
  p.bytes = p.off_ms + (long long)p.nlists * n * 2 * 4;
  return p;
}

template <int TC, int TQ, int WM, int WN>
int tl_launch_tiles(const TlPlan& p, const float* x, const float* w, const float* bias, int n, int v, int h, int k,
                    const long long* gold, unsigned long long* part, float* ms, float* gold_score, hipStream_t st) {
  const dim3 grid(p.qtiles * p.chunks), block(64 * WM * WN);
#define K3M_TL_LAUNCH(KP)                                                                                          \
  hipLaunchKernelGGL((topk_logits_tile_kernel<TC, TQ, WM, WN, KP>), grid, block, 0, st, x, w, bias, n, v, h, k, gold, \
                     p.tiles, p.tiles_per_chunk, p.qtiles, part, ms, gold_score)
  if (k <= 16) K3M_TL_LAUNCH(16);
  else K3M_TL_LAUNCH(32);
#undef K3M_TL_LAUNCH
  K3M_CHECK_LAUNCH();
  return 0;
}

bool tl_args_ok(int n, int v, int h, int k, int chunks) {
  return n >= 0 && v >= 1 && k >= 1 && k <= TL_MAXK && h >= 4 && h <= 4096 && h % 4 == 0 && chunks >= 0;
}

}  // namespace

extern "C" int k3m_topk_logits_ws_bytes(int n, int v, int h, int k, int chunks, long long* bytes) {
  K3M_ARG(bytes && tl_args_ok(n, v, h, k, chunks));
  *bytes = tl_plan(n, v, k, chunks).bytes;
  return 0;
}

extern "C" int k3m_topk_logits(const float* x, const float* w, const float* bias, int n, int v, int h, int k,
                               const long long* gold, int chunks, float* scores, long long* idx, float* lse,
                               float* gold_score, void* ws, long long ws_bytes, hipStream_t st) {
  K3M_ARG(tl_args_ok(n, v, h, k, chunks));
  if (n == 0) return 0;
  K3M_ARG(x && w && scores && idx && lse && (gold != nullptr) == (gold_score != nullptr));
  K3M_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0);
  const TlPlan p = tl_plan(n, v, k, chunks);
  K3M_ARG(ws && ws_bytes >= p.bytes);
  char* wsb = static_cast<char*>(ws);
  unsigned long long* part = reinterpret_cast<unsigned long long*>(wsb);
  float* ms = reinterpret_cast<float*>(wsb + p.off_ms);
  const int rc = p.small ? tl_launch_tiles<256, 64, 2, 2>(p, x, w, bias, n, v, h, k, gold, part, ms, gold_score, st)
                         : tl_launch_tiles<128, 128, 1, 4>(p, x, w, bias, n, v, h, k, gold, part, ms, gold_score, st);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(topk_logits_merge_kernel, dim3(n), dim3(64 * TL_MERGE_NW), 0, st, part, ms, p.nlists, n, k,
                     scores, idx, lse);
  K3M_CHECK_LAUNCH();
  return 0;
}
