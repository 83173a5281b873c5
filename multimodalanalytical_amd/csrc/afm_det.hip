// Deterministic mode (include/afm_hip.h, "Deterministic mode"): the atomic-free forms of the training step's reductions.
//   - afm_gemm_group_det: weight gradients.  Every k-chunk of a split-K plan stores its fp32 partial tile (and its partial column
//     sums) to its own slab of a workspace; a reduce launch adds the slabs in chunk order into C (and a_colsum).  The plan -- kernel,
//     split count, chunk length -- is a function of the call's shapes, dtypes and operand alignment only.  16-bit operands of the
//     grouped-wgrad shapes run the grouped MFMA kernel with its slab epilogue (afm_gemm_mfma_impl.h, tn256_unit<true>); everything
//     else (fp32, split pairs, small or ragged shapes) runs k_wgrad_det below, a plain fp32 FMA tile kernel.
//   - afm_colsum_det: block partials over fixed row chunks, then the same reduce.
//   - afm_scatter_add_rows_det: one wave per (table row, 64 columns), the rows of dout that map to it summed sequentially in ascending
//     row order.
#include <algorithm>
#include <functional>
#include <vector>
#include "afm_det.h"

// ------------------------------------------------------------------------------------------ fixed-order reduces
// The order is a function of P alone: with P <= DET_GROUP the partials are added left to right; beyond, groups of DET_GROUP
// consecutive partials are first summed (8 at a time left to right, the four eights then as (a + b) + (c + d)) IN PLACE into the
// group's first partial, and those group sums are added left to right.
#define DET_GROUP 32
__device__ __forceinline__ int64_t det_elem(int64_t i, int cols, int ldp) {
  const int64_t r = i / cols;
  return r * ldp + (i - r * cols);
}

// pass 1: grid (elements / 64, groups); lane = element, wave w sums partials g * 32 + 8 w .. + 7
__global__ __launch_bounds__(256) void k_det_group(float* __restrict__ parts, int P, int64_t pstride, int rows, int cols, int ldp) {
  __shared__ float sm[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t e = (int64_t)blockIdx.x * 64 + lane;
  const bool in = e < (int64_t)rows * cols;
  const int64_t off = in ? det_elem(e, cols, ldp) : 0;
  const int p0 = blockIdx.y * DET_GROUP + 8 * w;
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = (in && p0 + k < P) ? parts[(int64_t)(p0 + k) * pstride + off] : 0.f;
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) t = __fadd_rn(t, v[k]);
  sm[w][lane] = t;
  __syncthreads();                 // every read of the group is done before its first partial is overwritten
  if (w == 0 && in) parts[(int64_t)blockIdx.y * DET_GROUP * pstride + off] = __fadd_rn(__fadd_rn(sm[0][lane], sm[1][lane]), __fadd_rn(sm[2][lane], sm[3][lane]));
}

// pass 2 (or the only pass): out = (accumulate ? out : 0) + sum of the P partials left to right
__global__ __launch_bounds__(256) void k_det_sum(const float* __restrict__ parts, int P, int64_t pstride, int rows, int cols, int ldp,
                                                 float* __restrict__ out, int ldo, int accumulate) {
  const int64_t total = (int64_t)rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / cols), c = (int)(i - (int64_t)r * cols);
    const float* p = parts + (int64_t)r * ldp + c;
    float t = 0.f;
    int s = 0;
    for (; s + 4 <= P; s += 4) {     // four loads in flight, added in order
      const float a = p[(int64_t)s * pstride], b = p[(int64_t)(s + 1) * pstride], c2 = p[(int64_t)(s + 2) * pstride], d = p[(int64_t)(s + 3) * pstride];
      t = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(t, a), b), c2), d);
    }
    for (; s < P; ++s) t = __fadd_rn(t, p[(int64_t)s * pstride]);
    float* o = out + (int64_t)r * ldo + c;
    *o = accumulate ? __fadd_rn(*o, t) : t;
  }
}

// (parts is overwritten when P > DET_GROUP)
int afm_det_sum_launch(const float* parts_, int P, int64_t pstride, int rows, int cols, int ldp, float* out, int ldo, int accumulate,
                       hipStream_t st) {
  float* parts = (float*)parts_;
  if (!parts || !out || P < 1 || rows < 0 || cols < 0) return AFM_ERR_ARG;
  const int64_t total = (int64_t)rows * cols;
  if (total == 0) return AFM_OK;
  if (P > DET_GROUP) {
    const int groups = (P + DET_GROUP - 1) / DET_GROUP;
    AFM_LAUNCH(k_det_group, dim3((unsigned)((total + 63) / 64), groups), dim3(256), 0, st, parts, P, pstride, rows, cols, ldp);
    P = groups;
    pstride *= DET_GROUP;
  }
  int64_t g = (total + 255) / 256;
  if (g > 4096) g = 4096;
  AFM_LAUNCH(k_det_sum, dim3((unsigned)g), dim3(256), 0, st, parts, P, pstride, rows, cols, ldp, out, ldo, accumulate);
  return AFM_OK;
}

__global__ __launch_bounds__(256) void k_det_total(const float* __restrict__ parts, int P, int nv, float* __restrict__ out) {
  __shared__ float sm[4][256];
  const int t = threadIdx.x;
  for (int v = 0; v < nv; ++v) {
    float a = 0.f;
    for (int p = t; p < P; p += 256) a = __fadd_rn(a, parts[(int64_t)p * nv + v]);
    sm[v][t] = a;
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s)
      for (int v = 0; v < nv; ++v) sm[v][t] = __fadd_rn(sm[v][t], sm[v][t + s]);
    __syncthreads();
  }
  if (t < nv) out[t] = __fadd_rn(out[t], sm[t][0]);
}

int afm_det_total_launch(const float* parts, int P, int nv, float* out, hipStream_t st) {
  if (!parts || !out || P < 1 || nv < 1 || nv > 4) return AFM_ERR_ARG;
  AFM_LAUNCH(k_det_total, dim3(1), dim3(256), 0, st, parts, P, nv, out);
  return AFM_OK;
}

// ------------------------------------------------------------------------------------------ weight gradients
__device__ __forceinline__ int det_glu_deint(int n, int f) { return ((n >> 3) << 2) + (n & 3) + ((n >> 2) & 1) * f; }

// grid (N / 64, M / 64, ksplit): the 64 x 64 tile of C = A^T B (A: K x M, B: K x N, row-major) over token rows
// [ks * kchunk, min(K, (ks + 1) * kchunk)), in order, stored to slab ks (rows de-interleaved as C's); the blocks of the first
// column tile also store the chunk's column sums of A to colsum slab ks.
#define WD_T 64
#define WD_BK 16
template <typename TA, typename TB>
__global__ __launch_bounds__(256) void k_wgrad_det(const TA* __restrict__ A, const TB* __restrict__ B, int M, int N, int K, int lda,
                                                   int ldb, int kchunk, int glu_f, float* __restrict__ slab,
                                                   float* __restrict__ cs_slab) {
  __shared__ float As[WD_BK][WD_T], Bs[WD_BK][WD_T];
  const int t = threadIdx.x, tm = t >> 4, tn = t & 15;
  const int m0 = blockIdx.y * WD_T, n0 = blockIdx.x * WD_T, ks = blockIdx.z;
  const int kbeg = ks * kchunk, kend = min(K, kbeg + kchunk);
  const bool do_cs = cs_slab != nullptr && blockIdx.x == 0;
  float acc[4][4] = {};
  float cs = 0.f;
  for (int k0 = kbeg; k0 < kend; k0 += WD_BK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = t + 256 * q, kk = e >> 6, cc = e & 63;
      const int k = k0 + kk;
      As[kk][cc] = (k < kend && m0 + cc < M) ? ld_rc(A, k, m0 + cc, lda) : 0.f;
      Bs[kk][cc] = (k < kend && n0 + cc < N) ? ld_rc(B, k, n0 + cc, ldb) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < WD_BK; ++kk) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = As[kk][tm * 4 + i]; b[i] = Bs[kk][tn * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    if (do_cs && t < WD_T)
      for (int kk = 0; kk < WD_BK; ++kk) cs = __fadd_rn(cs, As[kk][t]);
    __syncthreads();
  }
  float* out = slab + (int64_t)ks * M * N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + tm * 4 + i;
    if (m >= M) continue;
    const int row = glu_f ? det_glu_deint(m, glu_f) : m;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + tn * 4 + j;
      if (n < N) out[(int64_t)row * N + n] = acc[i][j];
    }
  }
  if (do_cs && t < WD_T && m0 + t < M) cs_slab[(int64_t)ks * M + (glu_f ? det_glu_deint(m0 + t, glu_f) : m0 + t)] = cs;
}

// defined in afm_gemm_mfma.hip / afm_gemm_mfma_f16.hip
bool afm_gemm_tn_group_eligible(const afm_gemm_desc* d);
bool afm_gemm_tn_group_eligible_f16(const afm_gemm_desc* d);
int afm_gemm_tn_group_det_launch(const afm_gemm_desc* const* ds, const int* ksplit, float* const* slab, float* const* cs_slab, int count,
                                 hipStream_t st);
int afm_gemm_tn_group_det_launch_f16(const afm_gemm_desc* const* ds, const int* ksplit, float* const* slab, float* const* cs_slab,
                                     int count, hipStream_t st);

extern "C" int afm_last_hint(void);

namespace {
struct DetPlan {
  int kind;        // 0 generic (k_wgrad_det), 1 grouped MFMA bf16, 2 grouped MFMA fp16
  int ksplit;      // k-chunks
  int parts;       // partial column sums per column of A
  int64_t slab_floats, cs_floats;
};

// The weight-gradient form the det path takes: C (fp32) = op, no epilogue.  (Null pointers pass here: the size query may run on
// placeholders.  Operand ALIGNMENT does enter the plan, through the grouped kernel's eligibility: query with the real pointers.)
bool det_wgrad_form(const afm_gemm_desc* d) {
  if (!d->transA || d->transB || d->c_dtype != AFM_F32) return false;
  if (d->M <= 0 || d->N <= 0 || d->K < 0 || d->bias || d->residual || d->pre_act || d->act != AFM_ACT_NONE || d->drop.p > 0.f) return false;
  if (d->a_dtype < AFM_F32 || d->a_dtype > AFM_F16 || d->b_dtype < AFM_F32 || d->b_dtype > AFM_F16) return false;
  const int ca = d->a_dtype == AFM_BF16X2 ? 2 : 1, cb = d->b_dtype == AFM_BF16X2 ? 2 : 1;
  if (d->lda < ca * d->M || d->ldb < cb * d->N || d->ldc < d->N) return false;
  if ((ca == 2 && (d->lda & 1)) || (cb == 2 && (d->ldb & 1))) return false;
  if (d->glu_rows && ((d->glu_rows & 3) || 2 * d->glu_rows != d->M)) return false;
  return true;
}

// Chunk length (64-token k-steps) shared by one grouped launch: the greedy schedule of its units on 256 workgroup slots, each unit
// charged its steps + 40 (ring fill, slab store), over splits of the longest problem into 1 .. 16 chunks of >= 16 steps; a finer
// split has to pay by 3 %.  The same estimate as the default grouped plan (afm_gemm_tn_group_launch) without its environment
// overrides and its cache: a function of the group's shapes only.
int det_group_chunk(const int* ntile, const int* steps, int n) {
  int max_steps = 0;
  for (int i = 0; i < n; ++i) max_steps = std::max(max_steps, steps[i]);
  int chunk = max_steps;
  double best = 1e30;
  for (int ks0 = 1; ks0 <= 16; ++ks0) {
    const int c = (max_steps + ks0 - 1) / ks0;
    if (c < 16) break;
    std::vector<int> finish(256, 0);
    int makespan = 0;
    for (int i = 0; i < n; ++i) {
      int ks = (steps[i] + c - 1) / c;
      const int per = (steps[i] + ks - 1) / ks;
      ks = (steps[i] + per - 1) / per;
      for (int u = 0; u < ntile[i] * ks; ++u) {
        std::pop_heap(finish.begin(), finish.end(), std::greater<int>());
        finish.back() += per + 40;
        makespan = std::max(makespan, finish.back());
        std::push_heap(finish.begin(), finish.end(), std::greater<int>());
      }
    }
    if (makespan < best * 0.97) { best = makespan; chunk = c; }
  }
  return chunk;
}

// Shape-only plans of a det call: no occupancy query, device attribute or environment variable takes part.  The grouped MFMA
// problems are taken in order, up to 8 per launch and operand type (as afm_gemm_group_det launches them), and split by their
// launch's shared chunk length; the rest are planned one by one.
void det_plan_all(const afm_gemm_desc* descs, int count, std::vector<DetPlan>& plans) {
  plans.assign(count, DetPlan{});
  int members[2][8], ng[2] = {0, 0};
  auto flush = [&](int t) {
    if (!ng[t]) return;
    int ntile[8], steps[8];
    for (int k = 0; k < ng[t]; ++k) {
      const afm_gemm_desc* d = descs + members[t][k];
      ntile[k] = ((d->M + 255) / 256) * ((d->N + 255) / 256);
      steps[k] = d->K / 64;                              // 64-token k-steps (K % 64 == 0 there)
    }
    const int chunk = det_group_chunk(ntile, steps, ng[t]);
    for (int k = 0; k < ng[t]; ++k) {
      DetPlan& p = plans[members[t][k]];
      const afm_gemm_desc* d = descs + members[t][k];
      int ks = (steps[k] + chunk - 1) / chunk;
      const int per = (steps[k] + ks - 1) / ks;
      ks = (steps[k] + per - 1) / per;
      p.ksplit = ks;
      p.parts = ks * ((d->N + 255) / 256) * 4;
    }
    ng[t] = 0;
  };
  for (int i = 0; i < count; ++i) {
    const afm_gemm_desc* d = descs + i;
    DetPlan& p = plans[i];
    afm_gemm_desc e = *d;                   // the grouped kernel's eligibility, whatever the caller's accumulate / variant / algo
    e.accumulate = 1; e.reserved = 0; e.algo = AFM_ALGO_AUTO;
    const bool f16 = afm_gemm_tn_group_eligible_f16(&e), b16 = !f16 && afm_gemm_tn_group_eligible(&e);
    if (f16 || b16) {
      const int t = f16 ? 1 : 0;
      p.kind = t + 1;
      members[t][ng[t]++] = i;
      if (ng[t] == 8) flush(t);
      continue;
    }
    // the fp32 FMA kernel: >= 1 024 tokens per chunk, at most 64 chunks and 2^24 slab floats (skinny problems -- the patch
    // embedding's -- split furthest)
    const int64_t mn = (int64_t)d->M * d->N;
    const int cap = (int)std::max<int64_t>(1, std::min<int64_t>(64, ((int64_t)1 << 24) / mn));
    int ks = d->K / 1024;
    ks = ks < 1 ? 1 : (ks > cap ? cap : ks);
    const int kchunk = ((d->K + ks - 1) / ks + WD_BK - 1) / WD_BK * WD_BK;
    ks = d->K > 0 ? (d->K + kchunk - 1) / kchunk : 1;
    p.kind = 0;
    p.ksplit = ks;
    p.parts = ks;
  }
  flush(0);
  flush(1);
  for (int i = 0; i < count; ++i) {
    DetPlan& p = plans[i];
    const afm_gemm_desc* d = descs + i;
    p.slab_floats = ((int64_t)p.ksplit * d->M * d->N + 3) & ~(int64_t)3;
    p.cs_floats = d->a_colsum ? (((int64_t)p.parts * d->M + 3) & ~(int64_t)3) : 0;
  }
}

int wgrad_det_generic(const afm_gemm_desc* d, const DetPlan& p, float* slab, float* cs_slab, hipStream_t st) {
  const int kchunk = d->K > 0 ? ((d->K + p.ksplit - 1) / p.ksplit + WD_BK - 1) / WD_BK * WD_BK : WD_BK;
  const dim3 grid((d->N + WD_T - 1) / WD_T, (d->M + WD_T - 1) / WD_T, p.ksplit);
  float* cs = d->a_colsum ? cs_slab : nullptr;
#define WD_LAUNCH(TA_) AFM_DT_SWITCH(d->b_dtype, TB_, AFM_LAUNCH((k_wgrad_det<TA_, TB_>), grid, dim3(256), 0, st, (const TA_*)d->A, \
                                     (const TB_*)d->B, d->M, d->N, d->K, d->lda, d->ldb, kchunk, d->glu_rows, slab, cs))
  AFM_DT_SWITCH(d->a_dtype, TA_, WD_LAUNCH(TA_));
#undef WD_LAUNCH
  return AFM_OK;
}
}  // namespace

extern "C" int64_t afm_gemm_group_det_ws_floats(const afm_gemm_desc* descs, int32_t count) {
  if (count < 0 || (count > 0 && !descs)) return -1;
  for (int i = 0; i < count; ++i)
    if (!det_wgrad_form(descs + i)) return -1;
  std::vector<DetPlan> plans;
  det_plan_all(descs, count, plans);
  int64_t n = 0;
  for (const DetPlan& p : plans) n += p.slab_floats + p.cs_floats;
  return n;
}

extern "C" int afm_gemm_group_det(const afm_gemm_desc* descs, int32_t count, float* ws, int64_t ws_floats, void* stream) {
  if (count < 0 || (count > 0 && !descs)) return AFM_ERR_ARG;
  for (int i = 0; i < count; ++i) {
    if (!descs[i].A || !descs[i].B || !descs[i].C) return AFM_ERR_ARG;
    if (!det_wgrad_form(descs + i)) return AFM_ERR_UNSUPPORTED;
  }
  std::vector<DetPlan> plans;             // planned once: the size check and the launches below use the same plan
  det_plan_all(descs, count, plans);
  int64_t need = 0;
  for (const DetPlan& p : plans) need += p.slab_floats + p.cs_floats;
  if (need > 0 && (!ws || ws_floats < need || ((uintptr_t)ws & 15))) return AFM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  afm_note_hint(0);
  int hint = 0;
  // 1. partials: the grouped MFMA problems in launches of up to 8 per operand type, the rest one generic launch each
  const afm_gemm_desc* grp[2][8];
  int gks[2][8];
  float* gslab[2][8];
  float* gcs[2][8];
  int ng[2] = {0, 0};
  auto flush = [&](int t) -> int {
    if (!ng[t]) return AFM_OK;
    const int r = t ? afm_gemm_tn_group_det_launch_f16(grp[t], gks[t], gslab[t], gcs[t], ng[t], st)
                    : afm_gemm_tn_group_det_launch(grp[t], gks[t], gslab[t], gcs[t], ng[t], st);
    const int s = afm_last_hint();
    if (s < 0) hint = -1; else if (s > 0 && hint == 0) hint = 1;
    ng[t] = 0;
    return r;
  };
  float* w = ws;
  for (int i = 0; i < count; ++i) {
    const afm_gemm_desc* d = descs + i;
    const DetPlan& p = plans[i];
    float* slab = w;
    float* cs = w + p.slab_floats;
    w += p.slab_floats + p.cs_floats;
    if (p.kind == 0) {
      if (d->k_live) hint = -1;
      const int r = wgrad_det_generic(d, p, slab, cs, st);
      if (r != AFM_OK) return r;
      continue;
    }
    const int t = p.kind - 1;
    grp[t][ng[t]] = d; gks[t][ng[t]] = p.ksplit; gslab[t][ng[t]] = slab; gcs[t][ng[t]] = cs;
    if (++ng[t] == 8) { const int r = flush(t); if (r != AFM_OK) return r; }
  }
  for (int t = 0; t < 2; ++t) { const int r = flush(t); if (r != AFM_OK) return r; }
  // 2. the slabs, in chunk order, into C and a_colsum
  w = ws;
  for (int i = 0; i < count; ++i) {
    const afm_gemm_desc* d = descs + i;
    const DetPlan& p = plans[i];
    float* slab = w;
    float* cs = w + p.slab_floats;
    w += p.slab_floats + p.cs_floats;
    int r = afm_det_sum_launch(slab, p.ksplit, (int64_t)d->M * d->N, d->M, d->N, d->N, (float*)d->C, d->ldc, d->accumulate, st);
    if (r == AFM_OK && d->a_colsum) r = afm_det_sum_launch(cs, p.parts, d->M, 1, d->M, d->M, d->a_colsum, d->M, 1, st);
    if (r != AFM_OK) return r;
  }
  afm_note_hint(hint);
  afm_set_last_algo(count == 1 && plans[0].kind == 0 ? "wgrad_det" : "wgrad_det_group");
  return AFM_OK;
}

// ------------------------------------------------------------------------------------------ column sums
// grid (n / 64, gy): block (x, y) sums rows [y * chunk, (y + 1) * chunk) of its 64 columns (wave w takes rows w, w + 4, ..., the four
// wave sums added in wave order) and stores the sum to parts[y * n + c].
#define CS_ROWS 256
template <typename T>
__global__ __launch_bounds__(256) void k_colsum_det(const T* __restrict__ x, float* __restrict__ parts, int64_t rows, int n, int ld,
                                                    int64_t chunk) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.y * chunk;
  const int64_t r1 = r0 + chunk < rows ? r0 + chunk : rows;
  float acc = 0.f;
  if (c < n)
    for (int64_t r = r0 + w; r < r1; r += 4) acc = __fadd_rn(acc, ld_rc(x, r, c, ld));
  part[w][lane] = acc;
  __syncthreads();
  if (w == 0 && c < n) parts[(int64_t)blockIdx.y * n + c] = __fadd_rn(__fadd_rn(part[0][lane], part[1][lane]), __fadd_rn(part[2][lane], part[3][lane]));
}

static int colsum_det_chunks(int64_t rows) {
  int64_t gy = (rows + CS_ROWS - 1) / CS_ROWS;
  if (gy > 256) gy = 256;
  return gy < 1 ? 1 : (int)gy;
}

extern "C" int64_t afm_colsum_det_ws_floats(int64_t rows, int32_t n) {
  if (rows < 0 || n <= 0) return -1;
  return (int64_t)colsum_det_chunks(rows) * n;
}

extern "C" int afm_colsum_det(const void* x, float* out, int64_t rows, int32_t n, int32_t ld, int32_t dtype, int32_t accumulate, float* ws,
                              int64_t ws_floats, void* stream) {
  if (!x || !out || rows < 0 || n <= 0) return AFM_ERR_ARG;
  if (!ws || ws_floats < afm_colsum_det_ws_floats(rows, n)) return AFM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int gy = colsum_det_chunks(rows);
  const int64_t chunk = (rows + gy - 1) / gy;
  AFM_DT_SWITCH(dtype, T, AFM_LAUNCH(k_colsum_det<T>, dim3((n + 63) / 64, gy), dim3(256), 0, st, (const T*)x, ws, rows, n, ld, chunk));
  return afm_det_sum_launch(ws, gy, n, 1, n, n, out, n, accumulate, st);
}

// ------------------------------------------------------------------------------------------ embedding scatter-add
// order: the row indices 0 .. n-1 sorted STABLY by key(r) = (ids[r] == padding_idx ? V : clamped id), ascending; seg_end[i], at every
// sorted position i where the key changes (a segment start), is one past the segment's last position.  The wave of (sorted position i,
// 64-column chunk) that starts a table row's segment walks it in order:
// dtable[v, c] = (((dtable[v, c] + dout[r0, c] * s0) + dout[r1, c] * s1) ...) with r0 < r1 < ... the rows whose id maps to v, every
// product and sum rounded on its own (no contraction); the padding segment (key V) is skipped.  Eight rows are loaded ahead.
__device__ __forceinline__ int64_t det_key(int64_t id, int V, int64_t pad) { return id == pad ? V : (id < 0 ? 0 : (id >= V ? V - 1 : id)); }
__global__ __launch_bounds__(256) void k_scatter_add_rows_det(const int64_t* __restrict__ ids, const int64_t* __restrict__ order,
                                                              const int64_t* __restrict__ seg_end, const float* __restrict__ scale,
                                                              const float* __restrict__ dout, float* __restrict__ dtable, int64_t n, int d,
                                                              int V, int64_t pad) {
  const int lane = threadIdx.x & 63;
  const int nch = (d + 63) / 64;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t i = wv / nch;
  const int c = (int)(wv - i * nch) * 64 + lane;
  if (i >= n) return;
  auto row_at = [&](int64_t j) -> int64_t { const int64_t r = order[j]; return r < 0 ? 0 : (r >= n ? n - 1 : r); };
  const int64_t key = det_key(ids[row_at(i)], V, pad);
  if (key == V || (i > 0 && det_key(ids[row_at(i - 1)], V, pad) == key)) return;
  if (c >= d) return;
  const int64_t e = seg_end[i], end = e <= i ? i + 1 : (e > n ? n : e);      // (clamped: memory safety only)
  float* dst = dtable + key * (int64_t)d + c;
  float t = *dst;
  for (int64_t j0 = i; j0 < end; j0 += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (j0 + k < end) {
        const int64_t r = row_at(j0 + k);
        v[k] = dout[r * (int64_t)d + c];
        if (scale) v[k] = __fmul_rn(v[k], scale[r]);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (j0 + k < end) t = __fadd_rn(t, v[k]);
  }
  *dst = t;
}

extern "C" int afm_scatter_add_rows_det(const int64_t* ids, const int64_t* order, const int64_t* seg_end, const float* scale,
                                        const float* dout, float* dtable, int64_t n, int32_t d, int32_t V, int64_t padding_idx,
                                        void* stream) {
  if (!ids || !order || !seg_end || !dout || !dtable || n < 0 || d <= 0 || V <= 0) return AFM_ERR_ARG;
  if (n == 0) return AFM_OK;
  const int64_t waves = n * ((d + 63) / 64);
  AFM_LAUNCH(k_scatter_add_rows_det, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ids, order, seg_end, scale, dout, dtable,
             n, d, V, padding_idx);
  return AFM_OK;
}
