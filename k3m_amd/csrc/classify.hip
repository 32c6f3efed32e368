// Item-classification head: the reference's ClassificationHead (vilbert_k3m.py:2164-2183) over ONE
// item's final embedding e = c_final [B][H] and a C-way weighted, label-smoothed cross entropy:
//
//   x = dropout_p(e);  u = dense(x) (k3m_gemm);  h = dropout_p(tanh(u));  z = out_proj(h) (k3m_gemm) [B][C];
//   loss = F.cross_entropy(z, y, weight = w, ignore_index = -1, label_smoothing = eps)   (mean reduction)
//
// The element-wise kernels regenerate the dropout mask from (seed, off + b * H + c) and the tanh from u in the
// backward: no mask and no tanh(u) is stored.  The cross entropy is one workgroup per row (an online max /
// log-sum-exp pass, then dz written over z), between a one-workgroup pass that sums the divisor
// S = sum_{y_i != -1} w_{y_i} (it depends on every label) and a one-workgroup pass that sums the row losses: fixed
// orders, no atomics, so two runs give the same bits.  Bandwidth-bound and tiny (B x H and B x C elements).
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int EW_MAX_BLOCKS = 65536;   // the element-wise kernels stride over the rest

enum { OP_DROP = 0, OP_TANH_DROP = 1, OP_TANH_DROP_BWD = 2 };

// a: e (OP_DROP), dx (OP_DROP as the backward), u (the tanh forms); g: dh (OP_TANH_DROP_BWD only)
template <int OP>
__device__ __forceinline__ float ew_one(float a, float g, float keep) {
  if constexpr (OP == OP_DROP) return a * keep;
  const float t = tanhf(a);
  if constexpr (OP == OP_TANH_DROP) return t * keep;
  return g * keep * (1.f - t * t);
}

// out[i] = OP(a[i], g[i]) * keep(off + i), i < n.  VEC: four elements per thread through 16-byte accesses (the host
// checks H % 4 == 0 and the alignment), else one element per thread.  out may alias a or g.
template <int OP, bool VEC>
__global__ __launch_bounds__(NT) void ew_kernel(const float* a, const float* g, long long n, float p, uint64_t seed,
                                                uint64_t off, float* out) {
  const K3mDrop d = k3m_drop_init(seed, p);
  const long long stride = (long long)gridDim.x * NT;
  if constexpr (VEC) {
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4; i += stride) {
      const floatx4 va = reinterpret_cast<const floatx4*>(a)[i];
      floatx4 vg = {0.f, 0.f, 0.f, 0.f};
      if constexpr (OP == OP_TANH_DROP_BWD) vg = reinterpret_cast<const floatx4*>(g)[i];
      floatx4 vo;
#pragma unroll
      for (int j = 0; j < 4; ++j) vo[j] = ew_one<OP>(va[j], vg[j], k3m_drop(d, off + (uint64_t)(4 * i + j)));
      reinterpret_cast<floatx4*>(out)[i] = vo;
    }
  } else {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += stride) {
      const float vg = OP == OP_TANH_DROP_BWD ? g[i] : 0.f;
      out[i] = ew_one<OP>(a[i], vg, k3m_drop(d, off + (uint64_t)i));
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <int OP>
int ew_launch(const float* a, const float* g, int B, int H, float p, uint64_t seed, uint64_t off, float* out,
              hipStream_t st) {
  const long long n = (long long)B * H;
  if (n == 0) return 0;
  const bool vec = H % 4 == 0 && aligned16(a) && aligned16(out) && (OP != OP_TANH_DROP_BWD || aligned16(g));
  const long long want = ((vec ? n / 4 : n) + NT - 1) / NT;
  const int blocks = (int)(want < EW_MAX_BLOCKS ? want : EW_MAX_BLOCKS);
  if (vec)
    hipLaunchKernelGGL((ew_kernel<OP, true>), dim3(blocks), dim3(NT), 0, st, a, g, n, p, seed, off, out);
  else
    hipLaunchKernelGGL((ew_kernel<OP, false>), dim3(blocks), dim3(NT), 0, st, a, g, n, p, seed, off, out);
  K3M_CHECK_LAUNCH();
  return 0;
}

// block-wide minimum of an int for blockDim.x == NT; red holds NW ints; result broadcast to all
__device__ __forceinline__ int block_min_int(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  int s = red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) s = min(s, red[i]);
  return s;
}

// denom[0] = S = sum over the rows with a label in [0, C) of w[label] (1 without weights); denom[1] = sum_c w_c (C
// without weights).  One workgroup, thread-strided partial sums and the block tree: a fixed order.
__global__ __launch_bounds__(NT) void ce_denom_kernel(const long long* __restrict__ labels,
                                                      const float* __restrict__ weight, int rows, int C,
                                                      float* __restrict__ denom) {
  __shared__ float red[NW];
  float s = 0.f, ws = 0.f;
  for (int i = threadIdx.x; i < rows; i += NT) {
    const long long y = labels[i];
    if (y >= 0 && y < C) s += weight ? weight[y] : 1.f;
  }
  if (weight)
    for (int c = threadIdx.x; c < C; c += NT) ws += weight[c];
  s = block_sum<NW>(s, red);
  ws = block_sum<NW>(ws, red);
  if (threadIdx.x == 0) {
    denom[0] = s;
    denom[1] = weight ? ws : (float)C;
  }
}

// One workgroup per row.  The one body of ce_rows_kernel and ce_rows_fwd_kernel; GRAD = false: the forward-only
// form, no dz store (z is only read).
template <bool GRAD>
__device__ __forceinline__ void ce_row_body(float* z, long long ld, const long long* __restrict__ labels,
                                            const float* __restrict__ weight, float eps, int C,
                                            const float* __restrict__ denom, float* __restrict__ loss_rows,
                                            float* __restrict__ lse_out, int* __restrict__ pred) {
  __shared__ float red[NW];
  __shared__ int redi[NW];
  const int row = blockIdx.x;
  float* zr = z + (long long)row * ld;
  // online max / sum of exponentials, the lowest index of the maximum and sum_c w_c z_c, one read of the row
  float m = -INFINITY, s = 0.f, wz = 0.f;
  int bi = INT_MAX;
  for (int c = threadIdx.x; c < C; c += NT) {
    const float v = zr[c];
    if (bi == INT_MAX) {   // the lane's first element
      s = 1.f;
      m = v;
      bi = c;
    } else if (v > m) {
      s = s * expf(m - v) + 1.f;
      m = v;
      bi = c;
    } else {
      s += expf(v - m);
    }
    if (eps > 0.f) wz += (weight ? weight[c] : 1.f) * v;
  }
  const float M = block_max<NW>(m, red);
  const float S = block_sum<NW>(bi == INT_MAX ? 0.f : s * expf(m - M), red);
  if (eps > 0.f) wz = block_sum<NW>(wz, red);
  const int arg = block_min_int(bi != INT_MAX && m == M ? bi : INT_MAX, redi);
  const float lse = M + logf(S);
  const long long y = labels[row];
  const bool labelled = y >= 0 && y < C;
  const bool ok = labelled || y == -1;   // any other label: a NaN row, as align.hip's ok ? ... : NAN
  const float den = denom[0], wsum = denom[1];
  const float wy = labelled ? (weight ? weight[y] : 1.f) : 0.f;
  const float zy = labelled ? zr[y] : 0.f;   // read before any dz store (the stores follow a barrier below)
  const float a = (1.f - eps) * wy, b = eps / (float)C;
  if (threadIdx.x == 0) {
    float l = 0.f;
    if (!ok)
      l = NAN;
    else if (labelled && den > 0.f)
      l = a * (lse - zy) + (eps > 0.f ? b * (lse * wsum - wz) : 0.f);
    loss_rows[row] = l;
    lse_out[row] = lse;
    pred[row] = arg == INT_MAX ? 0 : arg;
  }
  if constexpr (GRAD) {
    __syncthreads();   // every lane holds zy before the row is overwritten
    const bool live = labelled && den > 0.f;
    const float inv = live ? 1.f / den : 0.f;
    for (int c = threadIdx.x; c < C; c += NT) {
      float dzc = 0.f;
      if (!ok) {
        dzc = NAN;
      } else if (live) {
        const float pc = expf(zr[c] - lse);
        dzc = a * (pc - (c == (int)y ? 1.f : 0.f));
        if (eps > 0.f) dzc += b * (pc * wsum - (weight ? weight[c] : 1.f));
        dzc *= inv;
      }
      zr[c] = dzc;
    }
  }
}

__global__ __launch_bounds__(NT) void ce_rows_kernel(float* z, long long ld, const long long* __restrict__ labels,
                                                     const float* __restrict__ weight, float eps, int C,
                                                     const float* __restrict__ denom, float* __restrict__ loss_rows,
                                                     float* __restrict__ lse, int* __restrict__ pred) {
  ce_row_body<true>(z, ld, labels, weight, eps, C, denom, loss_rows, lse, pred);
}

__global__ __launch_bounds__(NT) void ce_rows_fwd_kernel(const float* z, long long ld,
                                                         const long long* __restrict__ labels,
                                                         const float* __restrict__ weight, float eps, int C,
                                                         const float* __restrict__ denom,
                                                         float* __restrict__ loss_rows, float* __restrict__ lse,
                                                         int* __restrict__ pred) {
  ce_row_body<false>(const_cast<float*>(z), ld, labels, weight, eps, C, denom, loss_rows, lse, pred);
}

// loss = sum_i loss_rows[i] / S in a fixed order; S == 0 (no labelled row, or only zero-weight ones): 0, where torch
// divides 0 by 0.  A NaN row (a label outside {-1, 0 .. C-1}) stays a NaN loss in both cases.
__global__ __launch_bounds__(NT) void ce_loss_kernel(const float* __restrict__ loss_rows, int rows,
                                                     const float* __restrict__ denom, float* __restrict__ loss) {
  __shared__ float red[NW];
  float s = 0.f;
  for (int i = threadIdx.x; i < rows; i += NT) s += loss_rows[i];
  s = block_sum<NW>(s, red);
  if (threadIdx.x == 0) loss[0] = denom[0] > 0.f ? s / denom[0] : (s != s ? s : 0.f);
}

template <bool GRAD>
int ce_launch(float* z, long long ld, const long long* labels, const float* weight, float eps, int rows, int C,
              float* loss_rows, float* lse, float* loss, int* pred, float* denom, hipStream_t st) {
  K3M_ARG(rows >= 0 && C >= 1 && ld >= C && eps >= 0.f && eps < 1.f);
  if (rows == 0) return 0;
  K3M_ARG(z && labels && loss_rows && lse && loss && pred && denom);
  hipLaunchKernelGGL(ce_denom_kernel, dim3(1), dim3(NT), 0, st, labels, weight, rows, C, denom);
  K3M_CHECK_LAUNCH();
  if (GRAD)
    hipLaunchKernelGGL(ce_rows_kernel, dim3(rows), dim3(NT), 0, st, z, ld, labels, weight, eps, C, denom, loss_rows,
                       lse, pred);
  else
    hipLaunchKernelGGL(ce_rows_fwd_kernel, dim3(rows), dim3(NT), 0, st, z, ld, labels, weight, eps, C, denom,
                       loss_rows, lse, pred);
  K3M_CHECK_LAUNCH();
  hipLaunchKernelGGL(ce_loss_kernel, dim3(1), dim3(NT), 0, st, loss_rows, rows, denom, loss);
  K3M_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int k3m_cls_drop_fwd(const float* e, int B, int H, float p, uint64_t seed, uint64_t off, float* x,
                                hipStream_t st) {
  K3M_ARG(e && x && B >= 0 && H > 0 && p >= 0.f && p < 1.f);
  return ew_launch<OP_DROP>(e, nullptr, B, H, p, seed, off, x, st);
}

extern "C" int k3m_cls_drop_bwd(const float* dx, int B, int H, float p, uint64_t seed, uint64_t off, float* de,
                                hipStream_t st) {
  K3M_ARG(dx && de && B >= 0 && H > 0 && p >= 0.f && p < 1.f);
  return ew_launch<OP_DROP>(dx, nullptr, B, H, p, seed, off, de, st);
}

extern "C" int k3m_cls_tanh_drop_fwd(const float* u, int B, int H, float p, uint64_t seed, uint64_t off, float* h,
                                     hipStream_t st) {
  K3M_ARG(u && h && B >= 0 && H > 0 && p >= 0.f && p < 1.f);
  return ew_launch<OP_TANH_DROP>(u, nullptr, B, H, p, seed, off, h, st);
}

extern "C" int k3m_cls_tanh_drop_bwd(const float* dh, const float* u, int B, int H, float p, uint64_t seed,
                                     uint64_t off, float* du, hipStream_t st) {
  K3M_ARG(dh && u && du && B >= 0 && H > 0 && p >= 0.f && p < 1.f);
  return ew_launch<OP_TANH_DROP_BWD>(u, dh, B, H, p, seed, off, du, st);
}

extern "C" int k3m_cls_ce_fwd_bwd(float* z, long long ld, const long long* labels, const float* weight, float eps,
                                  int rows, int C, float* loss_rows, float* lse, float* loss, int* pred, float* denom,
                                  hipStream_t st) {
  return ce_launch<true>(z, ld, labels, weight, eps, rows, C, loss_rows, lse, loss, pred, denom, st);
}

extern "C" int k3m_cls_ce_fwd(const float* z, long long ld, const long long* labels, const float* weight, float eps,
                              int rows, int C, float* loss_rows, float* lse, float* loss, int* pred, float* denom,
                              hipStream_t st) {
  return ce_launch<false>(const_cast<float*>(z), ld, labels, weight, eps, rows, C, loss_rows, lse, loss, pred, denom,
                          st);
}
