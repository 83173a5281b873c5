// Spectrum augmentation of the training set (reference data/augmentations.py:12-39): Gaussian smoothing
// (scipy.ndimage.gaussian_filter1d, mode "reflect") and the horizontal shift (strided sub-sample + interp1d back
// onto 0..L-1), plus a plain copy so one launch can produce every row of an expanded set.
// One 256-thread workgroup per output row: the source row (reflect-extended for the smoothing) is staged in LDS,
// every point is evaluated in fp64 in the reference's order without contraction and rounded once to fp32.
// Algorithmic bytes per output row: 4 L read + 4 L written.
#include "afm_common.h"

#define AFM_AUG_MAX_L 4096
#define AFM_AUG_MAX_RADIUS 2048

struct AugOps {            // the op table, passed by value (<= AFM_AUG_MAX_OPS entries)
  int n;
  int kind[AFM_AUG_MAX_OPS], a[AFM_AUG_MAX_OPS], b[AFM_AUG_MAX_OPS];
};

// scipy's NI_EXTEND_REFLECT: d c b a | a b c d | d c b a, repeated with period 2L
__device__ __forceinline__ int reflect_index(int k, int L) {
  const int p = 2 * L;
  int m = k % p;
  m = m < 0 ? m + p : m;
  return m < L ? m : p - 1 - m;
}

__global__ __launch_bounds__(256) void k_spectra_augment(const float* __restrict__ table, int64_t N, int L,
                                                         const int64_t* __restrict__ src, const int32_t* __restrict__ op,
                                                         AugOps ops, const double* __restrict__ weights, int wcap,
                                                         float* __restrict__ out) {
#pragma clang fp contract(off)   // numpy / scipy multiply, then add: no fused multiply-add anywhere below
  extern __shared__ double aug_lds[];          // [wcap doubles: gauss weights][floats: the staged source row]
  double* sw = aug_lds;
  float* e = (float*)(aug_lds + wcap);
  const int64_t r = blockIdx.x;
  const int t = threadIdx.x;
  int64_t s = src[r];
  s = s < 0 ? 0 : (s >= N ? N - 1 : s);
  const float* row = table + s * L;
  float* dst = out + r * L;
  const int o = op[r];
  if (o < 0 || o >= ops.n) {                   // an op index outside the table: a visibly wrong row, never a stray read
    for (int j = t; j < L; j += 256) dst[j] = __builtin_nanf("");
    return;
  }
  const int kind = ops.kind[o];
  if (kind == AFM_AUG_GAUSS) {
    // gaussian_filter1d -> correlate1d, symmetric-kernel branch of scipy's NI_Correlate1D:
    //   out[i] = x[i] w0, then += (x[i-q] + x[i+q]) w_q for q = R down to 1 (the C loop runs jj = -R .. -1)
    const int R = ops.a[o];
    const double* w = weights + ops.b[o];
    for (int k = t; k <= R; k += 256) sw[k] = w[k];
    for (int k = t; k < L + 2 * R; k += 256) e[k] = row[reflect_index(k - R, L)];
    __syncthreads();
    for (int j = t; j < L; j += 256) {
      const float* c = e + j + R;
      double acc = (double)c[0] * sw[0];
      for (int q = R; q >= 1; --q) acc += ((double)c[-q] + (double)c[q]) * sw[q];
      dst[j] = (float)acc;
    }
  } else if (kind == AFM_AUG_HSHIFT) {
    // horizontal_shift_augment output i: y_k = x[i + n k] (k < m = L / n) on the knots np.linspace(0, L, m), evaluated at
    // 0..L-1 by interp1d, which hands a 1-D float64 y to np.interp: interval j with knot_j <= x < knot_j+1,
    // y_j itself on an exact knot, else slope * (x - knot_j) + y_j with slope = (y_j+1 - y_j) / (knot_j+1 - knot_j)
    const int n = ops.a[o], i = ops.b[o];
    const int m = L / n;
    for (int k = t; k < m; k += 256) e[k] = row[i + n * k];
    __syncthreads();
    const double step = (double)L / (double)(m - 1);       // linspace: arange(m) * (L / (m - 1)), last knot exactly L
    for (int j = t; j < L; j += 256) {
      const double x = (double)j;
      int k = (int)(x / step);
      k = k < 0 ? 0 : (k > m - 2 ? m - 2 : k);
      double lo = (double)k * step;
      double hi = k + 1 == m - 1 ? (double)L : (double)(k + 1) * step;
      while (k > 0 && lo > x) { --k; hi = lo; lo = (double)k * step; }
      while (k < m - 2 && hi <= x) { ++k; lo = hi; hi = k + 1 == m - 1 ? (double)L : (double)(k + 1) * step; }
      const double ylo = (double)e[k], yhi = (double)e[k + 1];
      double v;
      if (lo == x) {
        v = ylo;
      } else {
        const double slope = (yhi - ylo) / (hi - lo);
        v = slope * (x - lo) + ylo;
      }
      dst[j] = (float)v;
    }
  } else {                                     // AFM_AUG_COPY
    for (int j = t; j < L; j += 256) dst[j] = row[j];
  }
}

extern "C" int afm_spectra_augment(const float* table, int64_t N, int32_t L, const int64_t* src, const int32_t* op, int64_t M,
                                   const int32_t* op_desc_host, int32_t n_ops, const double* weights, int64_t n_weights,
                                   float* out, void* stream) {
  if (!table || !src || !op || !out || !op_desc_host || N <= 0 || L <= 0 || M < 0 || n_ops <= 0 || n_weights < 0)
    return AFM_ERR_ARG;
  if (L > AFM_AUG_MAX_L || n_ops > AFM_AUG_MAX_OPS || M > 0x7fffffff) return AFM_ERR_UNSUPPORTED;
  AugOps ops;
  ops.n = n_ops;
  int rmax = -1;
  for (int k = 0; k < n_ops; ++k) {
    const int kind = op_desc_host[3 * k], a = op_desc_host[3 * k + 1], b = op_desc_host[3 * k + 2];
    if (kind == AFM_AUG_GAUSS) {
      if (a < 0 || b < 0 || !weights || (int64_t)b + a + 1 > n_weights) return AFM_ERR_ARG;
      if (a > AFM_AUG_MAX_RADIUS) return AFM_ERR_UNSUPPORTED;
      rmax = a > rmax ? a : rmax;
    } else if (kind == AFM_AUG_HSHIFT) {
      // the reference's slice holds ceil(L / n) - 1 points against L // n knots: interp1d raises unless L % n != 0
      if (a < 1 || b < 0 || b >= a || L % a == 0 || L / a < 2) return AFM_ERR_ARG;
    } else if (kind != AFM_AUG_COPY) {
      return AFM_ERR_ARG;
    }
    ops.kind[k] = kind; ops.a[k] = a; ops.b[k] = b;
  }
  if (M == 0) return AFM_OK;
  const int wcap = rmax + 1;                                   // 0 without a gauss op
  const int ext = L + 2 * (rmax > 0 ? rmax : 0);
  const size_t lds = (size_t)wcap * sizeof(double) + (size_t)ext * sizeof(float);
  AFM_LAUNCH(k_spectra_augment, dim3((unsigned)M), dim3(256), lds, (hipStream_t)stream, table, N, (int)L, src, op, ops, weights,
             wcap, out);
  return AFM_OK;
}
