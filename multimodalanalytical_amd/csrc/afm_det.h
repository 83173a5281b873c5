// Deterministic mode: the fixed-order reduce launches behind every atomic-free (*_det) export.  Partials are written to a
// caller-provided workspace by the first launch; these add them up in index order, so the bits depend on the shapes only.
#pragma once
#include "afm_common.h"

// out[r * ldo + c] = (accumulate ? out[r * ldo + c] : 0) + (parts[0 * pstride + r * ldp + c] + ... + parts[(P-1) * pstride + ...]),
// the partials summed left to right starting from 0.
int afm_det_sum_launch(const float* parts, int P, int64_t pstride, int rows, int cols, int ldp, float* out, int ldo, int accumulate,
                       hipStream_t st);
// out[v] += sum over p of parts[p * nv + v] (v < nv <= 4), one workgroup, a fixed summation tree.
int afm_det_total_launch(const float* parts, int P, int nv, float* out, hipStream_t st);
