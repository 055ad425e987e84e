/* ORACLE (test infrastructure only -- never linked into the product library, never on the product path).
 * The exact sequential adjoint of the scalar-output Kalman logpdf (seq_kalman.c: seq_filter) with respect to the shared model
 * blocks: one source body (seq_adjoint_body.inc) over an arithmetic type, compiled twice. The long-double build (64-bit
 * mantissa on x86-64) is the reference the device's block gradients are held against at lengths the mpmath oracle
 * (lgssm_mp.py) cannot reach; the double build exists only to show how much rounding the long-double one removes.
 * Derived from seq_kalman_body.inc and lgssm_ref.py by hand (the derivation is the header of seq_adjoint_body.inc).
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define ADJ_MAXD 64      /* d <= 8: the modal engines' models; 8 < d <= 63: the wide-state engine's */
#define LOG2PI_L 1.8378770664093454835606594728112353L
#define RCAT_(a, b) a##_##b
#define RCAT(a, b) RCAT_(a, b)
#define RNAME(f) RCAT(f, RSUFFIX)

#define REAL long double
#define RSUFFIX ld
#define RLOG logl
#include "seq_adjoint_body.inc"
#undef REAL
#undef RSUFFIX
#undef RLOG

#define REAL double
#define RSUFFIX f64
#define RLOG log
#include "seq_adjoint_body.inc"
#undef REAL
#undef RSUFFIX
#undef RLOG

/* the mantissa of the reference's arithmetic: a platform whose long double is the 53-bit double must fail loudly in the tests */
int oracle_seq_adjoint_mant_dig(void) { return LDBL_MANT_DIG; }

/* use_double != 0: the double build. Return code 1: bad arguments, 2: innovation variance not positive, 3: out of memory. */
int oracle_seq_adjoint(int d, int64_t T, const double *A, const double *a, const double *Q, const double *H, const double *h, const double *R,
                       const double *y, const double *x0m, const double *x0P, int use_double, double *lml_out, double *gA, double *ga,
                       double *gQ, double *gH, double *gh, double *gR, double *gx0m, double *gx0P) {
    if (!A || !a || !Q || !H || !h || !R || !y || !x0m || !x0P || !lml_out || !gA || !ga || !gQ || !gH || !gh || !gR || !gx0m || !gx0P) return 1;
    return use_double ? seq_adjoint_f64(d, T, A, a, Q, H, *h, *R, y, x0m, x0P, lml_out, gA, ga, gQ, gH, gh, gR, gx0m, gx0P)
                      : seq_adjoint_ld(d, T, A, a, Q, H, *h, *R, y, x0m, x0P, lml_out, gA, ga, gQ, gH, gh, gR, gx0m, gx0P);
}
