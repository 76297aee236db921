/* rade_pack.h -- the host half of the matrix-core operand contract (rade_pack.c), for the files of the library: the fragment description, its three layouts and the
 * correlator basis.  The packers and table fills the tests call stay declared in rade_dev.h / rade_host.h; what is declared here crosses files inside the library only. */
#ifndef RADE_PACK_H
#define RADE_PACK_H

#include "rade_host.h"

#ifndef RD_HIDDEN
#define RD_HIDDEN __attribute__((visibility("hidden")))
#endif

/* A fragment is what the 64 lanes of one matrix instruction hold of an operand M[row][k], E consecutive k per lane.  THE LANE MAP, for every layout:
 *     row = R tile + lane % R,     k = (64 E / R) step + E (lane / R) + j,   j = 0 .. E - 1
 * and the element lies at out[((block planes + plane) 64 + lane) E + j], block = step tiles + tile (k-step-major) or tile steps + step (tile-major).
 * planes = 2: the high and the low binary16 plane of a block follow each other (rd_split2). */
enum { RD_KSTEP_MAJOR, RD_TILE_MAJOR };
typedef struct { int R, E, planes, order; } rd_frag;
extern RD_HIDDEN const rd_frag RD_FRAG_F32;    /* R 32, E 4: float32, k_gemm (v_mfma_f32_32x32x2_f32) */
extern RD_HIDDEN const rd_frag RD_FRAG_B16;    /* R 32, E 8: B operand of v_mfma_f32_32x32x16_f16, two planes (k_gemm16, k_encf_gemm) */
extern RD_HIDDEN const rd_frag RD_FRAG_A16;    /* R 16, E 8: A operand of v_mfma_f32_16x16x32_f16, two planes (the receiver's decoder, correlator, DFT and FIR) */
static inline int rd_frag_kstep(const rd_frag *L) { return 64 * L->E / L->R; }
static inline int rd_frag_tiles(const rd_frag *L, int N) { return (N + L->R - 1) / L->R; }
static inline long rd_frag_size(const rd_frag *L, int tiles, int steps) { return (long)steps * tiles * L->planes * 64 * L->E; }     /* in elements */

/* W[N][K] (K a multiple of the layout's k-step) as binary16 operands.  int8: ONE plane of the integers q of w = q row_scale[n], scale_out[R tiles] = the row scales (0 past N);
 * split: two planes of 2^10 w.  Return the size in halfs, or -1: not int8-exact (or no row scales) / a weight that does not fit the planes. */
RD_HIDDEN long rd_pack_int8(const rd_frag *L, const float *W, const float *row_scale, int N, int K, unsigned short *out, float *scale_out);
RD_HIDDEN long rd_pack_split(const rd_frag *L, const float *W, int N, int K, unsigned short *out);

/* the pilot correlator's basis (rade_pack.c: rd_corr_basis_fill): q[r][m] the 16 polynomials orthonormal on the 160 grid points, alpha = alr + j ali their expansion to the
 * 40 coarse frequencies.  A value the caller owns (37 KB: the heap, in the engine) and hands to the two fills and the check. */
typedef struct { double q[RD_NQ][RD_M], alr[RD_NQ][RD_NFC], ali[RD_NQ][RD_NFC]; } rd_corr_basis;
RD_HIDDEN void rd_corr_basis_fill(const rd_tables *T, rd_corr_basis *b);
RD_HIDDEN void rd_corrq16_fill(const rd_tables *T, const rd_corr_basis *b, unsigned short *out);
RD_HIDDEN void rd_corra16_fill(const rd_tables *T, const rd_corr_basis *b, unsigned short *out);
RD_HIDDEN double rd_corr_basis_check(const rd_tables *T, const rd_corr_basis *b);

#endif
