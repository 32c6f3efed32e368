// Initial-interactive fusion (pre_sampling_sequence, vilbert_k3m.py:2331-2374) and the pooling
// of the fused sequences (get_sequence_pooled_output_final :2404-2409).
//
// Layout: the three streams' ReLU outputs are packed as c[row, k*D + ch] (k = individual, cross1,
// cross2) — exactly torch.cat(feature_list, 2) — so the three gate scorers run as ONE GEMM
// against the contiguous [3D, 3D] weight view and the gate kernel reads score k of channel ch at
// column k*D + ch.
#include "common.h"

namespace {

template <typename T>
__global__ void relu_cat3_kernel(const T* x0, const T* x1, const T* x2, T* c, int rows, int d) {
  const long long n = (long long)rows * d;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / d, ch = e % d;
    T* o = c + r * 3 * d + ch;
    o[0] = from_f<T>(fmaxf(to_f(x0[e]), 0.f));
    o[d] = from_f<T>(fmaxf(to_f(x1[e]), 0.f));
    o[2 * d] = from_f<T>(fmaxf(to_f(x2[e]), 0.f));
  }
}

// SAVE = false: the forward-only form (k3m_gate_fwd with ys == idx == NULL), no ys / idx store in the kernel; the
// draws, the softmax arithmetic and the pick are the saving form's
template <typename T, bool SAVE = true>
__global__ void gate_fwd_kernel(const float* a, const T* c, const float* noise, float* ys, uint8_t* idx, T* out,
                                int rows, int d, uint64_t seed, uint64_t off) {
  const long long n = (long long)rows * d;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / d, ch = e % d;
    const long long b3 = r * 3 * d + ch;
    float z[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float g;
      if (noise) {
        g = noise[(r * 3 + k) * d + ch];
      } else {
        // gumbel(0,1) = -log(Exp(1)) = -log(-log(U))
        const float u = k3m_uniform(seed, off + (unsigned long long)(r * 3 + k) * d + ch);
        g = -logf(-logf(u));
      }
      z[k] = a[b3 + k * d] + g;
    }
    const float m = fmaxf(z[0], fmaxf(z[1], z[2]));
    const float e0 = expf(z[0] - m), e1 = expf(z[1] - m), e2 = expf(z[2] - m);
    const float inv = 1.f / (e0 + e1 + e2);
    const float y0 = e0 * inv, y1 = e1 * inv, y2 = e2 * inv;
    int k = 0;
    float best = y0;
    if (y1 > best) { best = y1; k = 1; }
    if (y2 > best) { k = 2; }
    if constexpr (SAVE) {
      ys[b3] = y0;
      ys[b3 + d] = y1;
      ys[b3 + 2 * d] = y2;
      idx[e] = (uint8_t)k;
    }
    out[e] = c[b3 + k * d];
  }
}

template <typename T>
__global__ void gate_bwd_kernel(const T* dout, const float* a, const T* c, const float* ys, const uint8_t* idx, T* dc,
                                T* dpre, int rows, int d) {
  const long long n = (long long)rows * d;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / d, ch = e % d;
    const long long b3 = r * 3 * d + ch;
    const float g = to_f(dout[e]);
    const int k = idx[e];
    float dy[3], y[3];
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      y[q] = ys[b3 + q * d];
      dy[q] = g * to_f(c[b3 + q * d]);
      s += y[q] * dy[q];
      dc[b3 + q * d] = from_f<T>(q == k ? g : 0.f);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float av = a[b3 + q * d];
      dpre[b3 + q * d] = from_f<T>(y[q] * (dy[q] - s) * av * (1.f - av));
    }
  }
}

template <typename T>
__global__ void relu_split3_bwd_kernel(const T* dc, const T* c, T* dx0, T* dx1, T* dx2, int rows, int d, int acc) {
  const long long n = (long long)rows * d;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / d, ch = e % d;
    const long long b3 = r * 3 * d + ch;
    T* dx[3] = {dx0, dx1, dx2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (!dx[k]) continue;
      const float g = to_f(c[b3 + k * d]) > 0.f ? to_f(dc[b3 + k * d]) : 0.f;
      dx[k][e] = from_f<T>(acc ? to_f(dx[k][e]) + g : g);
    }
  }
}

template <typename T>
__global__ void mean3_kernel(const T* x0, const T* x1, const T* x2, T* out, long long n) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
    out[e] = from_f<T>((to_f(x0[e]) + to_f(x1[e]) + to_f(x2[e])) / 3.f);
}
template <typename T>
__global__ void mean3_bwd_kernel(const T* dout, T* dx0, T* dx1, T* dx2, long long n, int acc) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const float g = to_f(dout[e]) / 3.f;
    T* dx[3] = {dx0, dx1, dx2};
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (dx[k]) dx[k][e] = from_f<T>(acc ? to_f(dx[k][e]) + g : g);
  }
}

// out[s, ch] (+)= scale * mean_{l >= start} x[s, l, ch]
template <typename T>
__global__ void seq_mean_kernel(const T* x, int nseq, int len, int start, int d, float scale, float* out, int acc) {
  const long long n = (long long)nseq * d;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const long long s = e / d, ch = e % d;
    float a = 0.f;
    for (int l = start; l < len; ++l) a += to_f(x[(s * len + l) * d + ch]);
    const float v = scale * (a / (float)(len - start));
    out[e] = acc ? out[e] + v : v;
  }
}
template <typename T>
__global__ void seq_mean_bwd_kernel(const float* dout, int nseq, int len, int start, int d, float scale, T* dx) {
  const long long n = (long long)nseq * len * d;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const long long ch = e % d, sl = e / d;
    const long long s = sl / len, l = sl % len;
    if (l < start) continue;
    dx[e] = from_f<T>(to_f(dx[e]) + scale * dout[s * d + ch] / (float)(len - start));
  }
}

int grid_for(long long n) { return (int)std::min<long long>((n + 255) / 256, 8192); }

// ---- soft gate (if_pre_sampling == 2) and interactive-only mean (== 3): streaming kernels, four
// elements per lane per trip (one 16-byte fp32 access, one 8-byte packed bf16 access), no atomics.
__device__ __forceinline__ void ld4(const float* p, float (&v)[4]) {
  const floatx4 t = *reinterpret_cast<const floatx4*>(p);
  v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}
__device__ __forceinline__ void ld4(const bf16_t* p, float (&v)[4]) {
  const uint2 t = *reinterpret_cast<const uint2*>(p);
  v[0] = __uint_as_float(t.x << 16);
  v[1] = __uint_as_float(t.x & 0xffff0000u);
  v[2] = __uint_as_float(t.y << 16);
  v[3] = __uint_as_float(t.y & 0xffff0000u);
}
__device__ __forceinline__ void st4(float* p, const float (&v)[4]) {
  floatx4 t;
  t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
  *reinterpret_cast<floatx4*>(p) = t;
}
__device__ __forceinline__ void st4(bf16_t* p, const float (&v)[4]) {
  uint2 t;
  t.x = (uint32_t)from_f<bf16_t>(v[0]).x | ((uint32_t)from_f<bf16_t>(v[1]).x << 16);
  t.y = (uint32_t)from_f<bf16_t>(v[2]).x | ((uint32_t)from_f<bf16_t>(v[3]).x << 16);
  *reinterpret_cast<uint2*>(p) = t;
}

// z = c * a ; n4 = element count / 4
template <typename T, typename Z>
__global__ void soft_scale_kernel(const T* c, const float* a, Z* z, long long n4) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float cv[4], av[4], zv[4];
    ld4(c + 4 * i, cv);
    ld4(a + 4 * i, av);
#pragma unroll
    for (int k = 0; k < 4; ++k) zv[k] = cv[k] * av[k];
    st4(z + 4 * i, zv);
  }
}

// dc = dz * a ; dpre = dz * c * a * (1 - a), fp32 and (dpre16 != NULL) its bf16 rounding
template <typename T>
__global__ void soft_scale_bwd_kernel(const T* dz, const T* c, const float* a, T* dc, float* dpre, bf16_t* dpre16,
                                      long long n4) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float gv[4], cv[4], av[4], dcv[4], dp[4];
    ld4(dz + 4 * i, gv);
    ld4(c + 4 * i, cv);
    ld4(a + 4 * i, av);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dcv[k] = gv[k] * av[k];
      dp[k] = gv[k] * cv[k] * av[k] * (1.f - av[k]);
    }
    st4(dc + 4 * i, dcv);
    st4(dpre + 4 * i, dp);
    if (dpre16) st4(dpre16 + 4 * i, dp);
  }
}

template <typename T>
__global__ void mean2_kernel(const T* x1, const T* x2, T* out, long long n4) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float u[4], v[4], o[4];
    ld4(x1 + 4 * i, u);
    ld4(x2 + 4 * i, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (u[k] + v[k]) * 0.5f;
    st4(out + 4 * i, o);
  }
}
template <typename T>
__global__ void mean2_bwd_kernel(const T* dout, T* dx1, T* dx2, long long n4, int acc) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float g[4];
    ld4(dout + 4 * i, g);
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] *= 0.5f;
    T* dx[2] = {dx1, dx2};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (!dx[q]) continue;
      float o[4];
      if (acc) {
        ld4(dx[q] + 4 * i, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] += g[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = g[k];
      }
      st4(dx[q] + 4 * i, o);
    }
  }
}

// ---- two-candidate gate (use_image = False: individual + one cross stream; pre_sampling_sequence with
// sequence_c1 = None).  c[row, k*D + ch], k in {individual, cross} = torch.cat(feature_list, 2).  Lane i of
// the flat index owns channels 4*(i % (D/4)) .. +3 of row i / (D/4); d4 = D / 4.
template <typename T>
__global__ void relu_cat2_kernel(const T* x0, const T* x1, T* c, long long n4, int d4) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / d4, b2 = (2 * r * d4 + i % d4) * 4;
    float u[4], v[4];
    ld4(x0 + 4 * i, u);
    ld4(x1 + 4 * i, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      u[k] = fmaxf(u[k], 0.f);
      v[k] = fmaxf(v[k], 0.f);
    }
    st4(c + b2, u);
    st4(c + b2 + 4 * d4, v);
  }
}

template <typename T, bool SAVE = true>   // SAVE as gate_fwd_kernel's
__global__ void gate2_fwd_kernel(const float* a, const T* c, const float* noise, float* ys, uint8_t* idx, T* out,
                                 long long n4, int d4, uint64_t seed, uint64_t off) {
  const long long d = 4LL * d4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / d4, ch = (i % d4) * 4, b2 = 2 * r * d + ch;
    float z0[4], z1[4], c0[4], c1[4], g0[4], g1[4], y0[4], y1[4], o[4];
    ld4(a + b2, z0);
    ld4(a + b2 + d, z1);
    ld4(c + b2, c0);
    ld4(c + b2 + d, c1);
    if (noise) {   // [rows, 2, D]: the same offsets as the scores
      ld4(noise + b2, g0);
      ld4(noise + b2 + d, g1);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // gumbel(0,1) = -log(Exp(1)) = -log(-log(U))
        g0[k] = -logf(-logf(k3m_uniform(seed, off + (unsigned long long)(b2 + k))));
        g1[k] = -logf(-logf(k3m_uniform(seed, off + (unsigned long long)(b2 + d + k))));
      }
    }
    uint32_t pick = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float s0 = z0[k] + g0[k], s1 = z1[k] + g1[k];
      const float m = fmaxf(s0, s1);
      const float e0 = expf(s0 - m), e1 = expf(s1 - m);
      const float inv = 1.f / (e0 + e1);
      y0[k] = e0 * inv;
      y1[k] = e1 * inv;
      const bool one = y1[k] > y0[k];   // the first maximum wins a tie
      pick |= (one ? 1u : 0u) << (8 * k);
      o[k] = one ? c1[k] : c0[k];
    }
    if constexpr (SAVE) {
      st4(ys + b2, y0);
      st4(ys + b2 + d, y1);
      *reinterpret_cast<uint32_t*>(idx + 4 * i) = pick;
    }
    st4(out + 4 * i, o);
  }
}

template <typename T>
__global__ void gate2_bwd_kernel(const T* dout, const float* a, const T* c, const float* ys, const uint8_t* idx, T* dc,
                                 T* dpre, long long n4, int d4) {
  const long long d = 4LL * d4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / d4, ch = (i % d4) * 4, b2 = 2 * r * d + ch;
    float g[4], a0[4], a1[4], c0[4], c1[4], y0[4], y1[4], dc0[4], dc1[4], p0[4], p1[4];
    ld4(dout + 4 * i, g);
    ld4(a + b2, a0);
    ld4(a + b2 + d, a1);
    ld4(c + b2, c0);
    ld4(c + b2 + d, c1);
    ld4(ys + b2, y0);
    ld4(ys + b2 + d, y1);
    const uint32_t pick = *reinterpret_cast<const uint32_t*>(idx + 4 * i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool one = (pick >> (8 * k)) & 0xffu;
      // softmax' over two candidates: y_q (dy_q - sum_j y_j dy_j) = +-y0 y1 (dy0 - dy1), dy_q = g c_q.  The
      // factored form has no cancellation against the sum, so a confident pick (y1 ~ 1e-6) keeps its
      // relative precision and the bf16 rounding of dpre is that of the exact value.
      const float t = y0[k] * y1[k] * (g[k] * (c0[k] - c1[k]));
      dc0[k] = one ? 0.f : g[k];
      dc1[k] = one ? g[k] : 0.f;
      p0[k] = t * a0[k] * (1.f - a0[k]);
      p1[k] = -t * a1[k] * (1.f - a1[k]);
    }
    st4(dc + b2, dc0);
    st4(dc + b2 + d, dc1);
    st4(dpre + b2, p0);
    st4(dpre + b2 + d, p1);
  }
}

template <typename T>
__global__ void relu_split2_bwd_kernel(const T* dc, const T* c, T* dx0, T* dx1, long long n4, int d4, int acc) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / d4, b2 = (2 * r * d4 + i % d4) * 4;
    T* dx[2] = {dx0, dx1};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (!dx[q]) continue;
      float g[4], cv[4], o[4];
      ld4(dc + b2 + 4LL * q * d4, g);
      ld4(c + b2 + 4LL * q * d4, cv);
      if (acc) {
        ld4(dx[q] + 4 * i, o);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] += cv[k] > 0.f ? g[k] : 0.f;
      st4(dx[q] + 4 * i, o);
    }
  }
}

// the vector accesses need the operand on a 4-element boundary of its type (NULL passes)
bool al4(const void* p, int dtype) { return ((uintptr_t)p & (dtype == K3M_BF16 ? 7u : 15u)) == 0; }

}  // namespace

#define DISPATCH_T(dtype, ...)      \
  if ((dtype) == K3M_F32) {         \
    using T = float;                \
    __VA_ARGS__;                    \
  } else if ((dtype) == K3M_BF16) { \
    using T = bf16_t;               \
    __VA_ARGS__;                    \
  } else {                          \
    return K3M_EINVAL;              \
  }

extern "C" int k3m_relu_cat3(const void* x0, const void* x1, const void* x2, void* c, int rows, int d, int dtype,
                             hipStream_t st) {
  K3M_ARG(x0 && x1 && x2 && c);
  const long long n = (long long)rows * d;
  if (n == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(relu_cat3_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)x0,
                                       (const T*)x1, (const T*)x2, (T*)c, rows, d));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_gate_fwd(const float* a, const void* c, const float* noise, float* ys, uint8_t* idx, void* out,
                            int rows, int d, uint64_t seed, uint64_t off, int dtype, hipStream_t st) {
  K3M_ARG(a && c && out);
  K3M_ARG((ys == nullptr) == (idx == nullptr));   // both saved, or the forward-only form
  const long long n = (long long)rows * d;
  if (n == 0) return 0;
  if (ys) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(gate_fwd_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, a, (const T*)c,
                                         noise, ys, idx, (T*)out, rows, d, seed, off));
  } else {
    DISPATCH_T(dtype, hipLaunchKernelGGL((gate_fwd_kernel<T, false>), dim3(grid_for(n)), dim3(256), 0, st, a,
                                         (const T*)c, noise, ys, idx, (T*)out, rows, d, seed, off));
  }
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_gate_bwd(const void* dout, const float* a, const void* c, const float* ys, const uint8_t* idx,
                            void* dc, void* dpre, int rows, int d, int dtype, hipStream_t st) {
  K3M_ARG(dout && a && c && ys && idx && dc && dpre);
  const long long n = (long long)rows * d;
  if (n == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(gate_bwd_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)dout, a,
                                       (const T*)c, ys, idx, (T*)dc, (T*)dpre, rows, d));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_relu_split3_bwd(const void* dc, const void* c, void* dx0, void* dx1, void* dx2, int rows, int d,
                                   int accumulate, int dtype, hipStream_t st) {
  K3M_ARG(dc && c);
  const long long n = (long long)rows * d;
  if (n == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(relu_split3_bwd_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)dc,
                                       (const T*)c, (T*)dx0, (T*)dx1, (T*)dx2, rows, d, accumulate));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_relu_cat2(const void* x0, const void* x1, void* c, int rows, int d, int dtype, hipStream_t st) {
  K3M_ARG(x0 && x1 && c && rows >= 0 && d >= 0 && d % 4 == 0);
  K3M_ARG(al4(x0, dtype) && al4(x1, dtype) && al4(c, dtype));
  const long long n4 = (long long)rows * d / 4;
  if (n4 == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(relu_cat2_kernel<T>, dim3(grid_for(n4)), dim3(256), 0, st, (const T*)x0,
                                       (const T*)x1, (T*)c, n4, d / 4));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_gate2_fwd(const float* a, const void* c, const float* noise, float* ys, uint8_t* idx, void* out,
                             int rows, int d, uint64_t seed, uint64_t off, int dtype, hipStream_t st) {
  K3M_ARG(a && c && out && rows >= 0 && d >= 0 && d % 4 == 0);
  K3M_ARG((ys == nullptr) == (idx == nullptr));   // both saved, or the forward-only form
  K3M_ARG(al4(a, K3M_F32) && al4(c, dtype) && al4(noise, K3M_F32) && al4(ys, K3M_F32) && al4(out, dtype) &&
          ((uintptr_t)idx & 3u) == 0);
  const long long n4 = (long long)rows * d / 4;
  if (n4 == 0) return 0;
  if (ys) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(gate2_fwd_kernel<T>, dim3(grid_for(n4)), dim3(256), 0, st, a, (const T*)c,
                                         noise, ys, idx, (T*)out, n4, d / 4, seed, off));
  } else {
    DISPATCH_T(dtype, hipLaunchKernelGGL((gate2_fwd_kernel<T, false>), dim3(grid_for(n4)), dim3(256), 0, st, a,
                                         (const T*)c, noise, ys, idx, (T*)out, n4, d / 4, seed, off));
  }
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_gate2_bwd(const void* dout, const float* a, const void* c, const float* ys, const uint8_t* idx,
                             void* dc, void* dpre, int rows, int d, int dtype, hipStream_t st) {
  K3M_ARG(dout && a && c && ys && idx && dc && dpre && rows >= 0 && d >= 0 && d % 4 == 0);
  K3M_ARG(al4(dout, dtype) && al4(a, K3M_F32) && al4(c, dtype) && al4(ys, K3M_F32) && al4(dc, dtype) &&
          al4(dpre, dtype) && ((uintptr_t)idx & 3u) == 0);
  const long long n4 = (long long)rows * d / 4;
  if (n4 == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(gate2_bwd_kernel<T>, dim3(grid_for(n4)), dim3(256), 0, st, (const T*)dout, a,
                                       (const T*)c, ys, idx, (T*)dc, (T*)dpre, n4, d / 4));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_relu_split2_bwd(const void* dc, const void* c, void* dx0, void* dx1, int rows, int d, int accumulate,
                                   int dtype, hipStream_t st) {
  K3M_ARG(dc && c && rows >= 0 && d >= 0 && d % 4 == 0);
  K3M_ARG(al4(dc, dtype) && al4(c, dtype) && al4(dx0, dtype) && al4(dx1, dtype));
  const long long n4 = (long long)rows * d / 4;
  if (n4 == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(relu_split2_bwd_kernel<T>, dim3(grid_for(n4)), dim3(256), 0, st, (const T*)dc,
                                       (const T*)c, (T*)dx0, (T*)dx1, n4, d / 4, accumulate));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_mean3(const void* x0, const void* x1, const void* x2, void* out, long long n, int dtype,
                         hipStream_t st) {
  K3M_ARG(x0 && x1 && x2 && out);
  if (n == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(mean3_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)x0,
                                       (const T*)x1, (const T*)x2, (T*)out, n));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_mean3_bwd(const void* dout, void* dx0, void* dx1, void* dx2, long long n, int accumulate, int dtype,
                             hipStream_t st) {
  K3M_ARG(dout);
  if (n == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(mean3_bwd_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)dout,
                                       (T*)dx0, (T*)dx1, (T*)dx2, n, accumulate));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_soft_scale(const void* c, const float* a, void* z, int rows, int d, int dtype, int z_dtype,
                              hipStream_t st) {
  K3M_ARG(c && a && z && rows >= 0 && d >= 0 && d % 4 == 0);
  K3M_ARG(z_dtype == K3M_F32 || z_dtype == K3M_BF16);
  K3M_ARG(al4(c, dtype) && al4(a, K3M_F32) && al4(z, z_dtype));
  const long long n4 = (long long)rows * 3 * d / 4;
  if (n4 == 0) return 0;
  if (z_dtype == K3M_F32) {
    DISPATCH_T(dtype, hipLaunchKernelGGL((soft_scale_kernel<T, float>), dim3(grid_for(n4)), dim3(256), 0, st,
                                         (const T*)c, a, (float*)z, n4));
  } else {
    DISPATCH_T(dtype, hipLaunchKernelGGL((soft_scale_kernel<T, bf16_t>), dim3(grid_for(n4)), dim3(256), 0, st,
                                         (const T*)c, a, (bf16_t*)z, n4));
  }
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_soft_scale_bwd(const void* dz, const void* c, const float* a, void* dc, float* dpre, void* dpre_bf16,
                                  int rows, int d, int dtype, hipStream_t st) {
  K3M_ARG(dz && c && a && dc && dpre && rows >= 0 && d >= 0 && d % 4 == 0);
  K3M_ARG(al4(dz, dtype) && al4(c, dtype) && al4(a, K3M_F32) && al4(dc, dtype) && al4(dpre, K3M_F32) &&
          al4(dpre_bf16, K3M_BF16));
  const long long n4 = (long long)rows * 3 * d / 4;
  if (n4 == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(soft_scale_bwd_kernel<T>, dim3(grid_for(n4)), dim3(256), 0, st, (const T*)dz,
                                       (const T*)c, a, (T*)dc, dpre, (bf16_t*)dpre_bf16, n4));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_mean2(const void* x1, const void* x2, void* out, long long n, int dtype, hipStream_t st) {
  K3M_ARG(x1 && x2 && out && n >= 0 && n % 4 == 0);
  K3M_ARG(al4(x1, dtype) && al4(x2, dtype) && al4(out, dtype));
  if (n == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(mean2_kernel<T>, dim3(grid_for(n / 4)), dim3(256), 0, st, (const T*)x1,
                                       (const T*)x2, (T*)out, n / 4));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_mean2_bwd(const void* dout, void* dx1, void* dx2, long long n, int accumulate, int dtype,
                             hipStream_t st) {
  K3M_ARG(dout && n >= 0 && n % 4 == 0);
  K3M_ARG(al4(dout, dtype) && al4(dx1, dtype) && al4(dx2, dtype));
  if (n == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(mean2_bwd_kernel<T>, dim3(grid_for(n / 4)), dim3(256), 0, st, (const T*)dout,
                                       (T*)dx1, (T*)dx2, n / 4, accumulate));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_seq_mean(const void* x, int nseq, int len, int start, int d, float scale, float* out,
                            int accumulate, int dtype, hipStream_t st) {
  K3M_ARG(x && out && len > start);
  const long long n = (long long)nseq * d;
  if (n == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(seq_mean_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)x, nseq,
                                       len, start, d, scale, out, accumulate));
  K3M_CHECK_LAUNCH();
  return 0;
}

extern "C" int k3m_seq_mean_bwd(const float* dout, int nseq, int len, int start, int d, float scale, void* dx,
                                int dtype, hipStream_t st) {
  K3M_ARG(dout && dx && len > start);
  const long long n = (long long)nseq * len * d;
  if (n == 0) return 0;
  DISPATCH_T(dtype, hipLaunchKernelGGL(seq_mean_bwd_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, dout, nseq, len,
                                       start, d, scale, (T*)dx));
  K3M_CHECK_LAUNCH();
  return 0;
}
