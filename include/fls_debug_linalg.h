/* ============================================================================
 * fls_debug_linalg.h -- test-only entry points of the device linear-algebra primitives (same shared library as fls_reg.h;
 * FLS_ABI_REVISION stays 9, this header has a revision of its own).  Each hook runs ONE routine of csrc/linalg_dev.hpp or
 * csrc/wave_solve.hpp -- the __forceinline__ routine itself, compiled with the flags of the kernels that call it -- on n
 * caller-supplied inputs, so that tests/test_gpu_linalg.py can compare it with the CPU oracle's restatement bit for bit instead of
 * through the 1e-4 pose tolerance of a whole Match.  Same shape as fls_debug_fullpiv_qr6 / fls_debug_ldlt6 (fls_reg.h):
 * plain host pointers, synchronous, FLS_ERR_INVALID on a NULL pointer or a negative n (checked before the device is looked at),
 * n == 0 is FLS_OK without a launch.  All matrices are column-major; all values are doubles.
 * ==========================================================================*/
#ifndef FLS_DEBUG_LINALG_H
#define FLS_DEBUG_LINALG_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_DEBUG_LINALG_REVISION 1

int fls_debug_linalg_revision(void);

/* plane_fit_5x3 (ColPivHouseholderQR<5x3>::solve, right-hand side the routine's own -1): A[n][15], x[n][3]; one lane per system. */
fls_status fls_debug_plane_fit_5x3(int device_id, const double* A, int n, double* x);

/* jacobi_svd3_v (JacobiSVD<3x3>: singular values, descending, and V): A[n][9], S[n][3], V[n][9]; one lane per system. */
fls_status fls_debug_svd3(int device_id, const double* A, int n, double* S, double* V);

/* lu6_solve_wave (PartialPivLU<6x6>: determinant, explicit inverse, inverse * b) with the LDS layout of the ICP / NDT tail:
 * H[n][36], b[n][6], det[n], inv[n][36], x[n][6]; one wave per system. */
fls_status fls_debug_lu6(int device_id, const double* H, const double* b, int n, double* det, double* inv, double* x);

/* so3_exp_dev and mat3_mul_dev as the Gauss-Newton tails call them: Rd = SO3Exp(v), R_Rd = R * Rd (the right-multiplicative ICP / NDT
 * update), Rd_R = Rd * R (the left-multiplicative point-to-plane update).  v[n][3], R[n][9], Rd / R_Rd / Rd_R [n][9]; one lane per system. */
fls_status fls_debug_so3(int device_id, const double* v, const double* R, int n, double* Rd, double* R_Rd, double* Rd_R);

/* wave_sum_dpp: total[r] = lane 63 of the 64-lane sum of v[r][0..63]; one wave per row. */
fls_status fls_debug_wave_sum(int device_id, const double* v, int n, double* total);

#ifdef __cplusplus
}
#endif
#endif
