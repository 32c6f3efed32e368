// Dynamic image attention (BertImageSelfAttention with config.dynamic_attention, vilbert_k3m.py:572-601):
//   pool   = sum_t(mask * txt) / sum_t(mask)            masked mean of the image stream's text partner
//   g      = 1 + sigmoid(dyLinear_{q,k}(pool))           [nseq, 2 Hv]; the GEMM is the ordinary Linear path
//   Q, K  *= g (broadcast over the R rows of a sequence); V untouched
//
// Four streaming / short-reduction kernels around that GEMM.  No atomics and a fixed summation order, so the
// results are bit-reproducible and deterministic mode needs no second form.  Every lane moves 16 bytes (4 fp32 or
// 8 bf16); accumulation is fp32.
//
// Block shape of the three reducing kernels: 256 threads = 4 waves; lane l of every wave owns column group
// blockIdx.y * 64 + l (VEC consecutive columns), wave w walks rows w, w + 4, ... of sequence blockIdx.x.  The four
// waves' partials meet in LDS and are summed in wave order.
#include "common.h"

namespace {

template <typename T> struct Vec;
template <> struct Vec<float> { static constexpr int N = 4; };
template <> struct Vec<bf16_t> { static constexpr int N = 8; };

__device__ __forceinline__ void ldv(const float* p, float (&v)[4]) {
  const floatx4 t = *reinterpret_cast<const floatx4*>(p);
  v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}
__device__ __forceinline__ void stv(float* p, const float (&v)[4]) {
  floatx4 t;
  t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
  *reinterpret_cast<floatx4*>(p) = t;
}
__device__ __forceinline__ void ldv(const bf16_t* p, float (&v)[8]) {
  const uint4 t = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void stv(bf16_t* p, const float (&v)[8]) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    w[i] = (uint32_t)from_f<bf16_t>(v[2 * i]).x | ((uint32_t)from_f<bf16_t>(v[2 * i + 1]).x << 16);
  *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}

constexpr int NW = 4;   // waves per block

// sum of the four waves' N-vectors in wave order; red holds NW * N * 64 floats, laid out [wave][k][lane]
// (lane-contiguous: no bank conflict).  Every thread of the block calls it.
template <int N>
__device__ __forceinline__ void waves_sum(float (&a)[N], float* red) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < N; ++k) red[(w * N + k) * 64 + l] = a[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    float s = red[k * 64 + l];
#pragma unroll
    for (int i = 1; i < NW; ++i) s += red[(i * N + k) * 64 + l];
    a[k] = s;
  }
}

// pool[s, :] = sum_t mask[s, t] * x[s * len + t, :] / sum_t mask[s, t];  inv_count[s] = 1 / sum_t mask[s, t].
// A sequence with no kept token (count 0) gets pool = 0 and inv_count = 0: nothing is divided by zero, and the
// backward then adds nothing to its rows.
template <typename T>
__global__ __launch_bounds__(256) void dyn_pool_fwd_kernel(const T* x, long long ldx, const float* mask, float* pool,
                                                           float* inv_count, int len, int h) {
  constexpr int N = Vec<T>::N;
  __shared__ float red[NW * N * 64];
  __shared__ float cred[NW];
  const int s = blockIdx.x, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int cg = blockIdx.y * 64 + l;
  const bool live = cg < h / N;
  const float* m = mask + (long long)s * len;
  float acc[N];
#pragma unroll
  for (int k = 0; k < N; ++k) acc[k] = 0.f;
  float cnt = 0.f;
  for (int t = w; t < len; t += NW) {   // t and mv are wave-uniform
    const float mv = m[t];
    cnt += mv;
    if (mv != 0.f && live) {
      float v[N];
      ldv(x + ((long long)s * len + t) * ldx + (long long)cg * N, v);
#pragma unroll
      for (int k = 0; k < N; ++k) acc[k] = fmaf(mv, v[k], acc[k]);
    }
  }
  if (l == 0) cred[w] = cnt;
  waves_sum<N>(acc, red);   // its barrier also publishes cred
  float c = cred[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) c += cred[i];
  const float ic = c > 0.f ? 1.f / c : 0.f;
  if (w == 0 && live) {
    float o[N];
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = acc[k] * ic;
    float* dst = pool + (long long)s * h + (long long)cg * N;
    stv(dst, reinterpret_cast<float(&)[4]>(o[0]));
    if constexpr (N == 8) stv(dst + 4, reinterpret_cast<float(&)[4]>(o[N - 4]));
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) inv_count[s] = ic;
}

// dx[s * len + t, :] += mask[s, t] * inv_count[s] * dpool[s, :]
template <typename T>
__global__ __launch_bounds__(256) void dyn_pool_bwd_kernel(const float* dpool, const float* mask, const float* inv_count,
                                                           T* dx, long long ldx, int len, int h) {
  constexpr int N = Vec<T>::N;
  const int s = blockIdx.x, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int cg = blockIdx.y * 64 + l;
  if (cg >= h / N) return;   // no barrier in this kernel
  const float ic = inv_count[s];
  if (ic == 0.f) return;
  const float* m = mask + (long long)s * len;
  float g[N];
  const float* src = dpool + (long long)s * h + (long long)cg * N;
  ldv(src, reinterpret_cast<float(&)[4]>(g[0]));
  if constexpr (N == 8) ldv(src + 4, reinterpret_cast<float(&)[4]>(g[N - 4]));
  for (int t = w; t < len; t += NW) {
    const float mv = m[t] * ic;
    if (mv == 0.f) continue;
    T* p = dx + ((long long)s * len + t) * ldx + (long long)cg * N;
    float v[N];
    ldv(p, v);
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = fmaf(mv, g[k], v[k]);
    stv(p, v);
  }
}

// qkv[s * rows + r, c] *= 1 + sigmoid(z[s, c]) for c < 2 hv (the Q and K column blocks; V, columns >= 2 hv, is
// not touched)
template <typename T>
__global__ __launch_bounds__(256) void dyn_scale_fwd_kernel(T* qkv, long long ld, const float* z, int rows, int hv) {
  constexpr int N = Vec<T>::N;
  const int s = blockIdx.x, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int cg = blockIdx.y * 64 + l;
  if (cg >= 2 * hv / N) return;
  float g[N];
  const float* zs = z + (long long)s * 2 * hv + (long long)cg * N;
  ldv(zs, reinterpret_cast<float(&)[4]>(g[0]));
  if constexpr (N == 8) ldv(zs + 4, reinterpret_cast<float(&)[4]>(g[N - 4]));
#pragma unroll
  for (int k = 0; k < N; ++k) g[k] = 1.f + sigmoid_f(g[k]);
  for (int r = w; r < rows; r += NW) {
    T* p = qkv + ((long long)s * rows + r) * ld + (long long)cg * N;
    float v[N];
    ldv(p, v);
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] *= g[k];
    stv(p, v);
  }
}

// S[s, c] = sum_r dqkv[s, r, c] * qkv[s, r, c] (qkv holds the GATED Q' / K' = g * Q / K), g = 1 + sig, sig = sigmoid(z):
//   dz[s, c] = (S / g) * sig * (1 - sig)       (= sum_r dQ' * Q * dg/dz, since Q = Q' / g and g is constant over r)
//   dqkv[s, r, c] *= g                         (gradient w.r.t. the ungated projection), c < 2 hv
template <typename T>
__global__ __launch_bounds__(256) void dyn_scale_bwd_kernel(T* dqkv, long long ldd, const T* qkv, long long ldq,
                                                            const float* z, float* dz, int rows, int hv) {
  constexpr int N = Vec<T>::N;
  __shared__ float red[NW * N * 64];
  const int s = blockIdx.x, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int cg = blockIdx.y * 64 + l;
  const bool live = cg < 2 * hv / N;
  float sig[N], g[N], acc[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { sig[k] = 0.f; g[k] = 1.f; acc[k] = 0.f; }
  if (live) {
    const float* zs = z + (long long)s * 2 * hv + (long long)cg * N;
    ldv(zs, reinterpret_cast<float(&)[4]>(sig[0]));
    if constexpr (N == 8) ldv(zs + 4, reinterpret_cast<float(&)[4]>(sig[N - 4]));
#pragma unroll
    for (int k = 0; k < N; ++k) {
      sig[k] = sigmoid_f(sig[k]);
      g[k] = 1.f + sig[k];
    }
    for (int r = w; r < rows; r += NW) {
      T* pd = dqkv + ((long long)s * rows + r) * ldd + (long long)cg * N;
      float d[N], q[N];
      ldv(pd, d);
      ldv(qkv + ((long long)s * rows + r) * ldq + (long long)cg * N, q);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        acc[k] = fmaf(d[k], q[k], acc[k]);
        d[k] *= g[k];
      }
      stv(pd, d);
    }
  }
  waves_sum<N>(acc, red);
  if (w == 0 && live) {
    float o[N];
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = acc[k] / g[k] * sig[k] * (1.f - sig[k]);
    float* dst = dz + (long long)s * 2 * hv + (long long)cg * N;
    stv(dst, reinterpret_cast<float(&)[4]>(o[0]));
    if constexpr (N == 8) stv(dst + 4, reinterpret_cast<float(&)[4]>(o[N - 4]));
  }
}

bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
int vec_of(int dtype) { return dtype == K3M_BF16 ? 8 : 4; }
bool dtype_ok(int dtype) { return dtype == K3M_F32 || dtype == K3M_BF16; }

}  // namespace

#define DISPATCH_T(dtype, ...)      \
  if ((dtype) == K3M_F32) {         \
    using T = float;                \
    __VA_ARGS__;                    \
  } else {                          \
    using T = bf16_t;               \
    __VA_ARGS__;                    \
  }

extern "C" int k3m_dyn_pool_fwd(const void* x, long long ldx, const float* mask, float* pool, float* inv_count,
                                int nseq, int len, int h, int dtype, hipStream_t st) {
  K3M_ARG(x && mask && pool && inv_count && dtype_ok(dtype) && nseq >= 0 && len >= 0 && h >= 0);
  const int n = vec_of(dtype);
  K3M_ARG(h % n == 0 && ldx >= h && ldx % n == 0 && al16(x) && al16(pool));
  if (nseq == 0 || h == 0) return 0;
  const dim3 grid(nseq, k3m_cdiv(h / n, 64));
  DISPATCH_T(dtype, hipLaunchKernelGGL(dyn_pool_fwd_kernel<T>, grid, dim3(256), 0, st, (const T*)x, ldx, mask, pool,
                                       inv_count, len, h));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_dyn_pool_bwd(const float* dpool, const float* mask, const float* inv_count, void* dx, long long ldx,
                                int nseq, int len, int h, int dtype, hipStream_t st) {
  K3M_ARG(dpool && mask && inv_count && dx && dtype_ok(dtype) && nseq >= 0 && len >= 0 && h >= 0);
  const int n = vec_of(dtype);
  K3M_ARG(h % n == 0 && ldx >= h && ldx % n == 0 && al16(dx) && al16(dpool));
  if (nseq == 0 || h == 0 || len == 0) return 0;
  const dim3 grid(nseq, k3m_cdiv(h / n, 64));
  DISPATCH_T(dtype, hipLaunchKernelGGL(dyn_pool_bwd_kernel<T>, grid, dim3(256), 0, st, dpool, mask, inv_count, (T*)dx,
                                       ldx, len, h));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_dyn_scale_fwd(void* qkv, long long ld, const float* z, int nseq, int rows, int hv, int dtype,
                                 hipStream_t st) {
  K3M_ARG(qkv && z && dtype_ok(dtype) && nseq >= 0 && rows >= 0 && hv >= 0);
  const int n = vec_of(dtype);
  K3M_ARG(hv % n == 0 && ld >= 2LL * hv && ld % n == 0 && al16(qkv) && al16(z));
  if (nseq == 0 || rows == 0 || hv == 0) return 0;
  const dim3 grid(nseq, k3m_cdiv(2 * hv / n, 64));
  DISPATCH_T(dtype, hipLaunchKernelGGL(dyn_scale_fwd_kernel<T>, grid, dim3(256), 0, st, (T*)qkv, ld, z, rows, hv));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_dyn_scale_bwd(void* dqkv, long long ldd, const void* qkv, long long ldq, const float* z, float* dz,
                                 int nseq, int rows, int hv, int dtype, hipStream_t st) {
  K3M_ARG(dqkv && qkv && z && dz && dtype_ok(dtype) && nseq >= 0 && rows >= 0 && hv >= 0);
  const int n = vec_of(dtype);
  K3M_ARG(hv % n == 0 && ldd >= 2LL * hv && ldd % n == 0 && ldq >= 2LL * hv && ldq % n == 0);
  K3M_ARG(al16(dqkv) && al16(qkv) && al16(z) && al16(dz));
  if (nseq == 0 || hv == 0) return 0;
  const dim3 grid(nseq, k3m_cdiv(2 * hv / n, 64));
  DISPATCH_T(dtype, hipLaunchKernelGGL(dyn_scale_bwd_kernel<T>, grid, dim3(256), 0, st, (T*)dqkv, ldd, (const T*)qkv,
                                       ldq, z, dz, rows, hv));
  K3M_CHECK_LAUNCH();
  return 0;
}
