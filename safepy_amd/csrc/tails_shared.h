// Device code shared by the two streaming two-sided tests: hyptails.hip (safe_hypergeom_tails, safe_hypergeom_outputs) and
// moments.hip (safe_moments_test).  One source copy; every translation unit that includes it launches its own instance
// (no relocatable device code: a kernel is launched from the TU that holds it).
#pragma once
#include "common.h"

namespace {

// neighborhood_size = A . nodes_not_nan (safe.py:587-588): one wave per row, the member list read coalesced
__global__ __launch_bounds__(256) void k_hyp_tails_nbr_size(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                            const uint8_t *__restrict__ row_flags, int64_t n, double *__restrict__ out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    int c = 0;
    for (int32_t e = row_ptr[i] + lane; e < row_ptr[i + 1]; e += 64) c += row_flags[col[e]] != 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    if (lane == 0) out[i] = static_cast<double>(c);
}

// NES and the binarisation of one cell (safe.py:546-554 without the 1 / P substitution, 468-470).  One side: decided on p
// itself (nes_p_cut, common.h), as every other path does; 'both': |nes| against -log10(threshold) in doubles.
__device__ __forceinline__ bool tails_nes(double pp, double pn, int sign_mode, double p_cut, double nes_threshold, double *nes_out) {
    const double ep = -log10(pp), en = -log10(pn);
    const double nes = sign_mode == SAFE_SIGN_HIGHEST ? ep : sign_mode == SAFE_SIGN_LOWEST ? en : ep - en;
    *nes_out = nes;
    return sign_mode == SAFE_SIGN_HIGHEST ? pp < p_cut
           : sign_mode == SAFE_SIGN_LOWEST ? pn < p_cut
                                           : (nes == nes) && (fabs(nes) > nes_threshold);
}

__global__ void k_hyp_tails_u32_to_f64(const unsigned int *__restrict__ in, double *__restrict__ out, int64_t count) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < count) out[i] = static_cast<double>(in[i]);
}

}  // namespace
