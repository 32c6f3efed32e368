// Link-prediction ranking: for every query q_i [Nq][H] the k nearest (or farthest) rows of the
// candidates c [Nc][H] by squared L2 distance, and the rank of one gold row over ALL eligible candidates, without
// the [Nq][Nc] score matrix ever leaving the chip.  The squared-L2 sibling of topk.hip, whose design it takes.  The
// score is
//     s(i, r) = sign * (2 q_i . c_r - |c_r|^2)        sign = +1 nearest first, -1 farthest first
// which orders the candidates of a query as -+|q_i - c_r|^2 does (|q_i|^2 is constant per query).
//
//  1. lp_prep_kernel    |q_i|^2 (one wave per row, fixed summation order) and the gathered gold rows G[i] = c[gold[i]].
//  2. lp_gold_kernel    the tile code of step 3 over G: workgroup b computes only the diagonal tile, the gold rows of
//                       query tile b against query tile b, and the diagonal lanes store s(i, gold[i]).  By the
//                       determinism note below these are the bits step 3 produces for that pair, so a candidate row
//                       bit-equal to the gold row ties with it exactly.
//  3. lp_tile_kernel    topk.hip's tile kernel: a workgroup owns TQ queries and one CHUNK of the candidates, streamed
//                       in TC-row tiles through the exact-f32 MFMA main loop with the candidates as the A (row)
//                       operand; |c_r|^2 comes from the staged registers (LpRowSquares).  Per lane, in registers: the
//                       running top-k as 64-bit keys (order bits of s) << 32 | (0xffffffff - row), kept sorted by a
//                       ballot-gated compare-exchange chain, and an integer count of the eligible rows that stand
//                       before the gold in the list's own strict total order
//                           before(a, b) = s_a > s_b or (s_a == s_b and a < b).
//                       Eligibility (the filtered setting): with group ids, row r is eligible for query i iff
//                       r == gold[i] or q_gid[i] < 0 or c_gid[r] != q_gid[i]; the tile's c_gid values are staged in
//                       LDS once per tile.
//  4. lp_merge_kernel   one workgroup per query merges the lane lists (2 x WM per chunk) into the sorted output and
//                       sums the lists' counts, in list order, into the rank.
//
// Determinism: dot is the MFMA's k-ordered fmaf chain over the whole of H for its (query, row) pair, |c_r|^2 a sum in
// an order that no tile shape changes, and s = sign * fmaf(2, dot, -|c|^2) + 0 rounds once: the bits of a score do
// not depend on tile, tiling, chunk or kernel.  (s, row) is a strict total order and the counts are integers, so d2,
// idx, gold_d2 and rank are bit-identical for every chunk count and both tilings.  No atomics; no two lanes store to
// one address.
#include "gemm_f32_tile.h"

#include <climits>

namespace {

using namespace K3M_F32_NS;

// k <= 32: the 64-entry list did not fit the register file (VGPR spills in the tile kernel), so it is not built
constexpr int LP_MAXK = 32;
constexpr int LP_MERGE_NW = 16;   // waves of a merge workgroup

__device__ __forceinline__ uint32_t lp_ord_bits(float s) {   // unsigned order == float order (no NaN)
  const uint32_t b = __float_as_uint(s);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float lp_unord_bits(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? o ^ 0x80000000u : ~o);
}
__device__ __forceinline__ bool lp_beats(float as, long long ai, float bs, long long bi) {
  return as > bs || (as == bs && ai < bi);
}
// one rounding (2 dot is exact), then an exact sign; + 0: -0 -> +0, one key per value
__device__ __forceinline__ float lp_score(float dot, float cc, float sign) { return sign * fmaf(2.f, dot, -cc) + 0.f; }
// |q|^2 - sign s: sign s is exact, one rounding
__device__ __forceinline__ float lp_d2(float qq, float s, float sign) { return fmaxf(qq - sign * s, 0.f); }

// qq[i] = |q_i|^2 and G[i] = c[gold[i]] (zeros without a gold row): one wave per query.
__global__ __launch_bounds__(256) void lp_prep_kernel(const float* __restrict__ q, const float* __restrict__ c,
                                                      const long long* __restrict__ gold, int nq, int nc, int H,
                                                      float* __restrict__ qq, float* __restrict__ G) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nq) return;
  const float* p = q + (long long)row * H;
  float ss = 0.f;
  for (int col = 4 * lane; col < H; col += 256) {
    const floatx4 v = *reinterpret_cast<const floatx4*>(p + col);
    ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  ss = wave_sum(ss);
  if (lane == 0) qq[row] = ss;
  if (!G) return;
  const long long g = gold[row];
  const bool has = g >= 0 && g < (long long)nc;
  const float* src = c + (has ? g : 0ll) * H;
  for (int col = 4 * lane; col < H; col += 256)
    *reinterpret_cast<floatx4*>(G + (long long)row * H + col) =
        has ? *reinterpret_cast<const floatx4*>(src + col) : floatx4{0.f, 0.f, 0.f, 0.f};
}

// Sum of squares of the candidate rows of a tile, from the main loop's staged registers, as topk.hip's RowSquares:
// thread t stages the 16-B piece (t + NT it) & 7 of row (t + NT it) >> 3 in every k-tile, ss[it] sums that piece's
// squares over the k-tiles in k order, and the row's eight pieces (eight consecutive lanes) meet by XOR shuffles.
// The order is the same for every tile shape and every position of the row in its tile.
template <int TC, int NT>
struct LpRowSquares {
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
  // cc[row of the tile] = |c|^2
  __device__ __forceinline__ void finish(float* cc) {
#pragma unroll
    for (int it = 0; it < NB; ++it) {
      float v = ss[it];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      const int idx = threadIdx.x + NT * it;
      if ((idx & 7) == 0) cc[idx >> 3] = v;
    }
  }
};

// gemm_f32_tile.h's main loop with one addition, as topk.hip's mainloop_sq: sq sees the thread's staged A registers
// of every k-tile, in k order.  Restated over the header's staging and LDS image because a hook in the header's
// own loop changed the schedule of every fp32 GEMM kernel.
template <int TC, int TQ, int WM, int WN>
__device__ __forceinline__ void lp_mainloop_sq(const float* __restrict__ A, const float* __restrict__ B, int H, int M,
                                               int N, int m0, int n0, float* smem, floatx16 (&acc)[TC / WM / 32][1],
                                               LpRowSquares<TC, 64 * WM * WN>& sq) {
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

// gs[i] = s(i, gold[i]) from the diagonal of (gathered gold rows of query tile b) x (query tile b).
template <int TC, int TQ, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN, 1) void lp_gold_kernel(const float* __restrict__ Q,
                                                                  const float* __restrict__ G, int Nq, int H,
                                                                  float sign, float* __restrict__ gs) {
  static_assert(TQ == 32 * WN && TQ <= TC, "the query tile's diagonal lies inside one candidate tile");
  constexpr int FM = TC / WM / 32;
  __shared__ __attribute__((aligned(16))) float smem[2 * (TC + TQ) * BK];
  __shared__ __attribute__((aligned(16))) float scc[TC];
  LpRowSquares<TC, 64 * WM * WN> sq;
  const int n0 = blockIdx.x * TQ, m0 = n0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5;
  const int wm = (w / WN) * (TC / WM), wn = (w % WN) * 32;
  const int q = n0 + wn + (lane & 31);
  floatx16 acc[FM][1];
  sq.clear();
  lp_mainloop_sq<TC, TQ, WM, WN>(G, Q, H, Nq, Nq, m0, n0, smem, acc, sq);
  sq.finish(scc);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int base = m0 + wm + 32 * i + 4 * h;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = base + (r & 3) + 8 * (r >> 2);
      if (row == q && q < Nq) gs[q] = lp_score(acc[i][0][r], scc[row - m0], sign);   // one lane per query
    }
  }
}

// part: [nlists][Nq][k] keys, list = (chunk * WM + wave row) * 2 + lane half; 0 = empty slot.
// cnt:  [nlists][Nq] the list's number of eligible rows before the gold.
template <int TC, int TQ, int WM, int WN, int KP, bool GID>
__global__ __launch_bounds__(64 * WM * WN, 1) void lp_tile_kernel(
    const float* __restrict__ Q, const float* __restrict__ Cm, int Nq, int Nc, int H, int k, float sign,
    const long long* __restrict__ gold, const float* __restrict__ gs, const long long* __restrict__ q_gid,
    const long long* __restrict__ c_gid, int tiles, int tiles_per_chunk, int qtiles,
    unsigned long long* __restrict__ part, int* __restrict__ cnt) {
  static_assert(TQ == 32 * WN, "one 32-query MFMA column block per wave");
  static_assert(TC <= 64 * WM * WN, "one group id per thread");
  constexpr int FM = TC / WM / 32;
  __shared__ __attribute__((aligned(16))) float smem[2 * (TC + TQ) * BK];
  __shared__ __attribute__((aligned(16))) float scc[TC];                   // |c|^2 of the tile's rows
  __shared__ __attribute__((aligned(16))) long long sgid[GID ? TC : 2];    // c_gid of the tile's rows
  LpRowSquares<TC, 64 * WM * WN> sq;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int chunk = id / qtiles, n0 = (id % qtiles) * TQ;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5;
  const int wmi = w / WN, wm = wmi * (TC / WM), wn = (w % WN) * 32;
  const int q = n0 + wn + (lane & 31);
  const bool qvalid = q < Nq;
  int grow = -1;          // the gold row of this query
  float gsv = INFINITY;   // its score: nothing stands before +inf
  if (gold && qvalid) {
    const long long g = gold[q];
    if (g >= 0 && g < (long long)Nc) {
      grow = (int)g;
      gsv = gs[q];
    }
  }
  long long qg = -1;   // < 0: every row is eligible
  if (GID && qvalid) qg = q_gid[q];
  const bool filt = qg >= 0;

  unsigned long long L[KP];
#pragma unroll
  for (int p = 0; p < KP; ++p) L[p] = 0ull;
  float thr_f = -INFINITY;   // score of the list's k-th entry
  int before = 0;

  const int t1 = min(tiles, (chunk + 1) * tiles_per_chunk);
  for (int t = chunk * tiles_per_chunk; t < t1; ++t) {
    const int m0 = t * TC;
    long long gv = -1;
    if (GID && (int)threadIdx.x < TC && m0 + (int)threadIdx.x < Nc) gv = c_gid[m0 + threadIdx.x];
    floatx16 acc[FM][1];
    sq.clear();
    lp_mainloop_sq<TC, TQ, WM, WN>(Cm, Q, H, Nc, Nq, m0, n0, smem, acc, sq);
    // (the main loop ended on a barrier, and every wave has passed one since it last read scc / sgid)
    sq.finish(scc);
    if (GID && (int)threadIdx.x < TC) sgid[threadIdx.x] = gv;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int base = m0 + wm + 32 * i + 4 * h;   // + (r & 3) + 8 (r >> 2): the row of accumulator r
      floatx4 ci[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) ci[g] = *reinterpret_cast<const floatx4*>(scc + (base - m0) + 8 * g);
      float sc[16];
      uint32_t cm = 0u;   // bit r: accumulator r is a candidate of the list
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = base + (r & 3) + 8 * (r >> 2);
        sc[r] = lp_score(acc[i][0][r], ci[r >> 2][r & 3], sign);
        bool ok = row < Nc;
        if (GID) ok = ok && !(filt && sgid[row - m0] == qg && row != grow);
        cm |= (uint32_t)(sc[r] >= thr_f && ok) << r;
        before += (ok && row != grow && (sc[r] > gsv || (sc[r] == gsv && row < grow))) ? 1 : 0;
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
        unsigned long long key = r < 16 ? ((unsigned long long)lp_ord_bits(s) << 32) | (0xffffffffu - row) : 0ull;
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
        thr_f = kth ? lp_unord_bits((uint32_t)(kth >> 32)) : -INFINITY;
      }
    }
  }
  if (qvalid) {
    const int list = (chunk * WM + wmi) * 2 + h;
    unsigned long long* o = part + ((long long)list * Nq + q) * k;
#pragma unroll
    for (int p = 0; p < KP; ++p)
      if (p < k) o[p] = L[p];
    cnt[(long long)list * Nq + q] = before;
  }
}

// One workgroup per query: wave w folds lists w, w + LP_MERGE_NW, ... into a sorted list held one entry per lane
// (lane p = rank p), the waves' lists meet in LDS and wave 0 folds them.  The last wave first sums the lists'
// counts: lane l takes lists l, l + 64, ... in order, then a fixed XOR-shuffle tree over the lanes.
__global__ __launch_bounds__(64 * LP_MERGE_NW) void lp_merge_kernel(
    const unsigned long long* __restrict__ part, const int* __restrict__ cnt, int nlists, int Nq, int Nc, int k,
    float sign, long long c_base, const float* __restrict__ qq, const long long* __restrict__ gold,
    const float* __restrict__ gs, float* __restrict__ d2, long long* __restrict__ idx, float* __restrict__ gold_d2,
    long long* __restrict__ rank) {
  __shared__ float ls[LP_MERGE_NW][LP_MAXK];
  __shared__ long long li[LP_MERGE_NW][LP_MAXK];
  const int q = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (w == LP_MERGE_NW - 1) {
    long long s = 0;
    for (int l = lane; l < nlists; l += 64) s += cnt[(long long)l * Nq + q];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
      const long long g = gold ? gold[q] : -1ll;
      const bool has = g >= 0 && g < (long long)Nc;
      rank[q] = has ? 1ll + s : 0ll;
      gold_d2[q] = has ? lp_d2(qq[q], gs[q], sign) : INFINITY;
    }
  }
  float ms = -INFINITY;       // this lane's entry of the running list; (-inf, LLONG_MAX) = empty
  long long mi = LLONG_MAX;
  // a sorted candidate list, entry t on lane t: entries are inserted until one no longer beats the k-th
  auto fold = [&](float cs_l, long long ci_l) {
    for (int t = 0; t < k; ++t) {
      const float cs = __shfl(cs_l, t, 64);
      const long long cidx = __shfl(ci_l, t, 64);
      if (!lp_beats(cs, cidx, __shfl(ms, k - 1, 64), __shfl(mi, k - 1, 64))) break;
      const bool b = lp_beats(cs, cidx, ms, mi);
      const bool pb = __shfl_up((int)b, 1, 64) != 0 && lane > 0;
      const float ps = __shfl_up(ms, 1, 64);
      const long long pi = __shfl_up(mi, 1, 64);
      if (b) {
        ms = pb ? ps : cs;
        mi = pb ? pi : cidx;
      }
    }
  };
  constexpr int AHEAD = 8;   // lists loaded before the first of them is folded
  for (int l0 = w; l0 < nlists; l0 += LP_MERGE_NW * AHEAD) {
    unsigned long long key[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const int l = l0 + u * LP_MERGE_NW;
      key[u] = (l < nlists && lane < k) ? part[((long long)l * Nq + q) * k + lane] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const float cs_l = key[u] ? lp_unord_bits((uint32_t)(key[u] >> 32)) : -INFINITY;
      const long long ci_l = key[u] ? (long long)(0xffffffffu - (uint32_t)key[u]) : LLONG_MAX;
      fold(cs_l, ci_l);
    }
  }
  if (lane < LP_MAXK) {
    ls[w][lane] = ms;
    li[w][lane] = mi;
  }
  __syncthreads();
  if (w != 0) return;
  for (int o = 1; o < LP_MERGE_NW; ++o) {
    const float cs_l = lane < LP_MAXK ? ls[o][lane] : -INFINITY;
    const long long ci_l = lane < LP_MAXK ? li[o][lane] : LLONG_MAX;
    fold(cs_l, ci_l);
  }
  if (lane < k) {
    const bool none = mi == LLONG_MAX;
    d2[(long long)q * k + lane] = none ? INFINITY : lp_d2(qq[q], ms, sign);
    idx[(long long)q * k + lane] = none ? -1ll : c_base + mi;
  }
}

// Tiling of one call, as topk.hip's.  Many queries: 128 x 128 tiles, four waves side by side on the queries.  Up to
// 64 queries: 256 candidate rows x 64 queries, 2 x 2 waves, so that the MFMAs are not spent on absent queries.
struct LpPlan {
  int small, tc, tq, wm, qtiles, tiles, chunks, tiles_per_chunk, nlists;
  long long off_gs, off_g, off_part, off_cnt, bytes;
};

constexpr int LP_NUM_CU = 256;
constexpr int LP_MAX_CHUNKS = 1024;

LpPlan lp_plan(int nq, int nc, int h, int k, int chunks) {
  LpPlan p;
  p.small = nq <= 64;
  p.tc = p.small ? 256 : 128;
  p.tq = p.small ? 64 : 128;
  p.wm = p.small ? 2 : 1;
  p.qtiles = k3m_cdiv(nq, p.tq);
  p.tiles = k3m_cdiv(nc, p.tc);
  if (chunks <= 0) chunks = k3m_cdiv(LP_NUM_CU, p.qtiles > 0 ? p.qtiles : 1);   // one workgroup per CU or more
  chunks = chunks > LP_MAX_CHUNKS ? LP_MAX_CHUNKS : chunks;
  chunks = chunks > p.tiles ? p.tiles : chunks;
  p.tiles_per_chunk = chunks > 0 ? k3m_cdiv(p.tiles, chunks) : 0;
  p.chunks = chunks > 0 ? k3m_cdiv(p.tiles, p.tiles_per_chunk) : 0;   // no empty chunk
  p.nlists = p.chunks * p.wm * 2;
  const long long nqp = ((long long)nq + 3) / 4 * 4;
  p.off_gs = nqp * 4;                                    // after |q|^2
  p.off_g = p.off_gs + nqp * 4;                          // the gathered gold rows [nq][h]
  p.off_part = p.off_g + (long long)nq * h * 4;          // h % 4 == 0: 16-B aligned
  p.off_cnt = p.off_part + (long long)p.nlists * nq * k * 8;
  p.bytes = p.off_cnt + (long long)p.nlists * nq * 4;
  return p;
}

struct LpArgs {
  const float *q, *c;
  int nq, nc, h, k;
  float sign;
  const long long *gold, *q_gid, *c_gid;
  const float* gs;
  unsigned long long* part;
  int* cnt;
};

template <int TC, int TQ, int WM, int WN>
int lp_launch_tiles(const LpPlan& p, const LpArgs& a, const float* G, float* gs, hipStream_t st) {
  const dim3 block(64 * WM * WN);
  if (a.gold) {
    hipLaunchKernelGGL((lp_gold_kernel<TC, TQ, WM, WN>), dim3(p.qtiles), block, 0, st, a.q, G, a.nq, a.h, a.sign, gs);
    K3M_CHECK_LAUNCH();
  }
  const dim3 grid(p.qtiles * p.chunks);
#define K3M_LP_LAUNCH(KP, GID)                                                                                      \
  hipLaunchKernelGGL((lp_tile_kernel<TC, TQ, WM, WN, KP, GID>), grid, block, 0, st, a.q, a.c, a.nq, a.nc, a.h, a.k, \
                     a.sign, a.gold, a.gs, a.q_gid, a.c_gid, p.tiles, p.tiles_per_chunk, p.qtiles, a.part, a.cnt)
  if (a.c_gid) {
    if (a.k <= 16) K3M_LP_LAUNCH(16, true);
    else K3M_LP_LAUNCH(32, true);
  } else {
    if (a.k <= 16) K3M_LP_LAUNCH(16, false);
    else K3M_LP_LAUNCH(32, false);
  }
#undef K3M_LP_LAUNCH
  K3M_CHECK_LAUNCH();
  return 0;
}

bool lp_args_ok(int nq, int nc, int h, int k, int chunks) {
  return nq >= 0 && nc >= 1 && k >= 1 && k <= LP_MAXK && h >= 4 && h <= 4096 && h % 4 == 0 && chunks >= 0;
}

}  // namespace

extern "C" int k3m_lp_rank_ws_bytes(int nq, int nc, int h, int k, int chunks, long long* bytes) {
  K3M_ARG(bytes && lp_args_ok(nq, nc, h, k, chunks));
  *bytes = lp_plan(nq, nc, h, k, chunks).bytes;
  return 0;
}

extern "C" int k3m_lp_rank(const float* q, const float* c, int nq, int nc, int h, int k, int farthest,
                           long long c_base, const long long* gold, const long long* q_gid, const long long* c_gid,
                           int chunks, float* d2, long long* idx, float* gold_d2, long long* rank, void* ws,
                           long long ws_bytes, hipStream_t st) {
  K3M_ARG(lp_args_ok(nq, nc, h, k, chunks) && (farthest == 0 || farthest == 1));
  K3M_ARG((q_gid != nullptr) == (c_gid != nullptr));
  if (nq == 0) return 0;
  K3M_ARG(q && c && d2 && idx && gold_d2 && rank);
  K3M_ARG(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0);
  const LpPlan p = lp_plan(nq, nc, h, k, chunks);
  K3M_ARG(ws && ws_bytes >= p.bytes);
  char* wsb = static_cast<char*>(ws);
  float* qq = reinterpret_cast<float*>(wsb);
  float* gs = reinterpret_cast<float*>(wsb + p.off_gs);
  float* G = gold ? reinterpret_cast<float*>(wsb + p.off_g) : nullptr;
  unsigned long long* part = reinterpret_cast<unsigned long long*>(wsb + p.off_part);
  int* cnt = reinterpret_cast<int*>(wsb + p.off_cnt);
  const float sign = farthest ? -1.f : 1.f;
  hipLaunchKernelGGL(lp_prep_kernel, dim3(k3m_cdiv(nq, 4)), dim3(256), 0, st, q, c, gold, nq, nc, h, qq, G);
  K3M_CHECK_LAUNCH();
  const LpArgs a{q, c, nq, nc, h, k, sign, gold, q_gid, c_gid, gs, part, cnt};
  const int rc = p.small ? lp_launch_tiles<256, 64, 2, 2>(p, a, G, gs, st) : lp_launch_tiles<128, 128, 1, 4>(p, a, G, gs, st);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(lp_merge_kernel, dim3(nq), dim3(64 * LP_MERGE_NW), 0, st, part, cnt, p.nlists, nq, nc, k, sign,
                     c_base, qq, gold, gs, d2, idx, gold_d2, rank);
  K3M_CHECK_LAUNCH();
  return 0;
}
