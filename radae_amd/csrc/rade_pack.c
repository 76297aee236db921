/*
 * rade_pack.c -- the host half of the matrix-core operand contract (plain C): every kernel that feeds the matrix cores reads operands the host has laid out in
 * fragment order, and this file is where that order is stated.  1. the binary16 codec, the two-plane split and the int8-exact test; 2. the fragment description
 * (rade_pack.h: rd_frag, the lane map), the ONE packing loop and its three value encodings; 3. the weight packers: a layout and a getter each; 4. the chunk-major
 * copies of the single-stream step kernel (not a fragment layout); 5. the pilot correlator's basis and the four constant operand tables of the receiver.
 */
#include "rade_pack.h"

#include <math.h>
#include <string.h>

#define PI_D 3.14159265358979323846

/* ---- 1. values ------------------------------------------------------------------------------------------------------------- */
/* float -> IEEE binary16 (round to nearest even, subnormals kept) and back */
static unsigned short f32_to_f16(float f)
{
    unsigned int x; memcpy(&x, &f, 4);
    const unsigned int sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (unsigned short)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0));
    if (x >= 0x477ff000u) return (unsigned short)(sign | 0x7c00u);                 /* rounds to >= 65520: infinity */
    if (x < 0x38800000u) {                                                         /* below 2^-14: subnormal half */
        if (x < 0x33000000u) return (unsigned short)sign;                          /* < 2^-25 */
        const int e = (int)(x >> 23);                                              /* biased float exponent, 102..112 */
        unsigned int m = (x & 0x7fffffu) | 0x800000u;
        const int shift = 126 - e;                                                 /* 14..24 */
        const unsigned int halfm = m >> shift, rem = m & ((1u << shift) - 1u), mid = 1u << (shift - 1);
        unsigned int r = halfm + ((rem > mid || (rem == mid && (halfm & 1u))) ? 1u : 0u);
        return (unsigned short)(sign | r);
    }
    unsigned int r = ((x - 0x38000000u) >> 13);
    const unsigned int rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) r++;
    return (unsigned short)(sign | r);
}
static float f16_to_f32(unsigned short h)
{
    const unsigned int sign = (unsigned int)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    unsigned int x;
    if (e == 0) {
        if (m == 0) x = sign;
        else { float f = (float)m * 5.9604644775390625e-08f; memcpy(&x, &f, 4); x |= sign; }      /* m * 2^-24 */
    } else if (e == 31) x = sign | 0x7f800000u | (m << 13);
    else x = sign | ((e + 112u) << 23) | (m << 13);
    float f; memcpy(&f, &x, 4); return f;
}
/* v = hi + lo to 22 bits: the two operand planes (the callers' power-of-two scale keeps the low plane out of binary16's subnormal range; the kernels' epilogues undo it) */
static void split2(float v, unsigned short *hi, unsigned short *lo) { *hi = f32_to_f16(v); *lo = f32_to_f16(v - f16_to_f32(*hi)); }

static int q_of(float w, float sc, float *q)
{   /* w = q * sc with integer |q| <= 127, exactly? */
    *q = 0.0f;
    if (w == 0.0f) return 0;
    if (sc == 0.0f) return -1;
    *q = rintf(w / sc);
    return (fabsf(*q) <= 127.0f && *q * sc == w) ? 0 : -1;
}

/* ---- 2. fragments (the lane map and the output index: rade_pack.h) ------------------------------------------------------------ */
const rd_frag RD_FRAG_F32 = { 32, 4, 1, RD_KSTEP_MAJOR }, RD_FRAG_B16 = { 32, 8, 2, RD_KSTEP_MAJOR }, RD_FRAG_A16 = { 16, 8, 2, RD_KSTEP_MAJOR };
static rd_frag frag_as(const rd_frag *L, int planes, int order) { rd_frag f = *L; f.planes = planes; f.order = order; return f; }
/* float32 operands pad K with zero columns to a whole k-step; the binary16 layouts take whole k-steps (their callers pad) */
static int frag_steps(const rd_frag *L, int K) { const int ks = rd_frag_kstep(L); return L->E == 4 ? (K + ks - 1) / ks : K / ks; }

/* a producer: *v = the logical element M[row][k] (0 <= row < N, 0 <= k < K); -1 = refuse */
typedef int (*elem_fn)(const void *ctx, int row, int k, double *v);
/* how a value is written: float32 | the two planes of scale * v (a power of two; refused unless below binary16's 65504: the high plane would be infinite, or v is
 * no number) | the integer q of v = q row_scale[row], exact in one binary16 plane (refused unless q_of says so) */
typedef struct { enum { WR_F32, WR_SPLIT, WR_INT8 } kind; double scale; const float *row_scale; } writer;

/* THE packing loop: M [N][K] through `get` into layout L, rows and columns past N, K as zeros; scale_out [R tiles] (WR_INT8) = the row scales, 0 past N.
 * Blocks are written in order, so a refusal leaves the blocks before it written.  Returns the size in elements, or -1.
 * Inlined into each producer: with the getter and the writer known there, the compiler folds the call and the switch (an engine open packs 7 M elements). */
static inline __attribute__((always_inline)) long frag_pack(const rd_frag *L, int N, int K, elem_fn get, const void *ctx, const writer *wr, void *out, float *scale_out)
{
    const int tiles = rd_frag_tiles(L, N), steps = frag_steps(L, K), kstep = rd_frag_kstep(L);
    if (wr->kind == WR_INT8) {
        if (!wr->row_scale) return -1;
        for (int n = 0; n < tiles * L->R; n++) scale_out[n] = n < N ? wr->row_scale[n] : 0.0f;
    }
    for (int block = 0; block < tiles * steps; block++) {
        const int step = L->order == RD_KSTEP_MAJOR ? block / tiles : block % steps, tile = L->order == RD_KSTEP_MAJOR ? block % tiles : block / steps;
        for (int lane = 0; lane < 64; lane++) {
            const int row = L->R * tile + lane % L->R, k0 = kstep * step + L->E * (lane / L->R);
            const size_t at = (((size_t)block * L->planes) * 64 + lane) * L->E;
            for (int j = 0; j < L->E; j++) {
                const int live = row < N && k0 + j < K;
                double v = 0.0;
                if (live && get(ctx, row, k0 + j, &v)) return -1;
                if (wr->kind == WR_F32) ((float *)out)[at + j] = (float)v;
                else if (wr->kind == WR_SPLIT) {
                    const float s = (float)(wr->scale * v);
                    unsigned short hi, lo, *o = (unsigned short *)out + at + j;
                    if (!(fabsf(s) < 65504.0f)) return -1;
                    split2(s, &hi, &lo);
                    o[0] = hi; o[64 * 8] = lo;                                     /* E = 8: the next plane of the block */
                } else {
                    float q = 0.0f;
                    if (live && q_of((float)v, wr->row_scale[row], &q)) return -1;
                    ((unsigned short *)out)[at + j] = f32_to_f16(q);
                }
            }
        }
    }
    return rd_frag_size(L, tiles, steps);
}

/* ---- 3. weights W[N][K], row-major ------------------------------------------------------------------------------------------ */
typedef struct { const float *W; int K; } weights;
static int weight_at(const void *ctx, int row, int k, double *v) { const weights *w = ctx; *v = w->W[(size_t)row * w->K + k]; return 0; }

long rd_pack_int8(const rd_frag *L, const float *W, const float *row_scale, int N, int K, unsigned short *out, float *scale_out)
{
    const rd_frag one = frag_as(L, 1, L->order); const weights w = { W, K }; const writer wr = { WR_INT8, 0.0, row_scale };
    return frag_pack(&one, N, K, weight_at, &w, &wr, out, scale_out);
}
long rd_pack_split(const rd_frag *L, const float *W, int N, int K, unsigned short *out)
{
    const weights w = { W, K }; const writer wr = { WR_SPLIT, 1024.0, NULL };                  /* |w| 2^10 must stay below 65504 */
    return frag_pack(L, N, K, weight_at, &w, &wr, out, NULL);
}

long rd_packed_size(int N, int K) { return rd_frag_size(&RD_FRAG_F32, rd_frag_tiles(&RD_FRAG_F32, N), frag_steps(&RD_FRAG_F32, K)); }
long rd_packed16_size(int N, int K) { return rd_frag_size(&RD_FRAG_B16, rd_frag_tiles(&RD_FRAG_B16, N), frag_steps(&RD_FRAG_B16, K)); }
long rd_packed16a_size(int N, int K) { return rd_frag_size(&RD_FRAG_A16, rd_frag_tiles(&RD_FRAG_A16, N), frag_steps(&RD_FRAG_A16, K)); }
long rd_pack_weights(const float *W, int N, int K, float *out)
{
    const weights w = { W, K }; const writer wr = { WR_F32, 0.0, NULL };
    return frag_pack(&RD_FRAG_F32, N, K, weight_at, &w, &wr, out, NULL);
}
/* k_gemm16 / k_encf_gemm (K a multiple of 16) and the receiver's in-kernel decoder (dq_gemm_tile: the weights as the A operand, K a multiple of 32) */
long rd_pack_weights_f16x2(const float *W, int N, int K, unsigned short *out) { return rd_pack_split(&RD_FRAG_B16, W, N, K, out); }
long rd_pack_weights_f16x2_a16(const float *W, int N, int K, unsigned short *out) { return rd_pack_split(&RD_FRAG_A16, W, N, K, out); }
long rd_pack_weights_q16(const float *W, const float *row_scale, int N, int K, unsigned short *out, float *scale_out) { return rd_pack_int8(&RD_FRAG_B16, W, row_scale, N, K, out, scale_out); }
long rd_pack_weights_q16_a16(const float *W, const float *row_scale, int N, int K, unsigned short *out, float *scale_out) { return rd_pack_int8(&RD_FRAG_A16, W, row_scale, N, K, out, scale_out); }

/* ---- 4. chunk-major copies for the single-stream step kernel (rade_core_step.hip): out[(c * Npad + n) * 8 + j] = W[n][8 c + j], K zero-padded to Kpad (a multiple
 *    of 8), rows to Npad (a multiple of 64).  _q16: the binary16 plane of the integers q of an int8 layer (w = q * row_scale[n] exactly); 0, or -1 when the layer
 *    is not int8-exact. */
int rd_chunkmajor_q16(const float *W, const float *row_scale, int N, int K, int Kpad, int Npad, unsigned short *out)
{
    if (!row_scale) return -1;
    for (int c = 0; c < Kpad / 8; c++)
        for (int n = 0; n < Npad; n++)
            for (int j = 0; j < 8; j++) {
                const int k = 8 * c + j;
                float q = 0.0f;
                if (n < N && k < K && q_of(W[(size_t)n * K + k], row_scale[n], &q)) return -1;
                out[((size_t)c * Npad + n) * 8 + j] = f32_to_f16(q);
            }
    return 0;
}
void rd_chunkmajor_f32(const float *W, int N, int K, int Kpad, int Npad, float *out)
{
    for (int c = 0; c < Kpad / 8; c++)
        for (int n = 0; n < Npad; n++)
            for (int j = 0; j < 8; j++) { const int k = 8 * c + j; out[((size_t)c * Npad + n) * 8 + j] = (n < N && k < K) ? W[(size_t)n * K + k] : 0.0f; }
}

/* ---- 5. the receiver's constant operand tables: A operands (RD_FRAG_A16), two planes, tile-major; their sizes are RD_*16_HALFS of rade_dev.h.  Their values are
 *    far below the planes' range: the fills cannot refuse. */
typedef struct { const rd_tables *T; const rd_corr_basis *b; } table_ctx;
static void table_fill(const rd_tables *T, const rd_corr_basis *b, int N, int K, elem_fn get, double scale, unsigned short *out)
{
    const rd_frag L = frag_as(&RD_FRAG_A16, 2, RD_TILE_MAJOR); const table_ctx c = { T, b }; const writer wr = { WR_SPLIT, scale, NULL };
    frag_pack(&L, N, K, get, &c, &wr, out, NULL);
}

/* ---- the pilot correlator in two stages: the basis and the two tables.  The device side -- operand layouts, scales and the product order, for the search,
 * check_pilots and whole-file acquisition alike -- is rade_corr2.h; the tables' geometry is RD_CORR_* of rade_dev.h ------------------------------------------------
 * p_w[m][f] = p[m] e^{j w_f m} for the 40 coarse frequencies |f| <= 50 Hz spans a window of 160 samples: the phase e^{j w_f (m - 79.5)} moves by at most
 * +-pi across it, i.e. as a function of x = (m - 79.5) / 80 it is band-limited to a time-bandwidth product of 2 and is reproduced to 1.7e-10 by its
 * projection on the first RD_NQ = 16 polynomials q_r orthonormal on the 160 grid points (14: 1.8e-8, 12: 1.5e-6):
 *     p_w[m][f] = sum_r alpha[r][f] s_r[m],   s_r[m] = p[m] q_r(x_m),   alpha[r][f] = e^{j w_f 79.5} sum_m q_r(x_m) e^{j w_f (m - 79.5)}
 * so Dt[t][f] = sum_m conj(rx[t + m]) p_w[m][f] = sum_r alpha[r][f] Mom_r[t] with the 16 "moments" Mom_r[t] = sum_m conj(rx[t + m]) s_r[m]: the big
 * product (K = 320 real) has 32 rows (two 16-row tiles) instead of 80 (five), and a second product with K = 32 expands the moments to the 40 frequencies.
 * On v_mfma_f32_16x16x32_f16: 2 x 10 x 3 + 5 x 5 = 85 matrix instructions per tile of 16 timings instead of 5 x 10 x 3 = 150.
 * rd_corrq16_table_fill: stage 1, the realified s_r (rows n' = 2 r + c', k = 2 m + c: {sr, si; si, -sr}[c'][c]), 2^12-scaled, [2 tiles][10 k-steps]
 * rd_corra16_table_fill: stage 2, A2[n = 2 f + c''][n'] = {ar, -ai; ai, ar} of alpha[r][f], 2^10-scaled, [5 tiles][1 k-step].  Its K axis is ordered the way
 *                        stage 1's accumulators lie in a lane (C layout of two 16-row tiles: lane group g holds rows 4 g .. 4 g + 3 of either tile), so that
 *                        the moments go from accumulator registers to B-operand registers without leaving the lane:
 *                        k-slot 8 g + j: n' = 4 g + j (j < 4), 16 + 4 g + (j - 4) (j >= 4) */
void rd_corr_basis_fill(const rd_tables *T, rd_corr_basis *b)
{
    /* orthonormal polynomials on x_m = (m - 79.5) / 80: Legendre recurrence, then two passes of modified Gram-Schmidt on the grid */
    double x[RD_M], (*q)[RD_M] = b->q;
    for (int m = 0; m < RD_M; m++) x[m] = ((double)m - 79.5) / 80.0;
    for (int m = 0; m < RD_M; m++) { q[0][m] = 1.0; q[1][m] = x[m]; }
    for (int r = 1; r + 1 < RD_NQ; r++)
        for (int m = 0; m < RD_M; m++) q[r + 1][m] = ((2.0 * r + 1.0) * x[m] * q[r][m] - (double)r * q[r - 1][m]) / (r + 1.0);
    for (int r = 0; r < RD_NQ; r++) {
        for (int pass = 0; pass < 2; pass++)
            for (int u = 0; u < r; u++) {
                double d = 0.0;
                for (int m = 0; m < RD_M; m++) d += q[u][m] * q[r][m];
                for (int m = 0; m < RD_M; m++) q[r][m] -= d * q[u][m];
            }
        double n2 = 0.0;
        for (int m = 0; m < RD_M; m++) n2 += q[r][m] * q[r][m];
        const double inv = 1.0 / sqrt(n2);
        for (int m = 0; m < RD_M; m++) q[r][m] *= inv;
    }
    for (int f = 0; f < RD_NFC; f++) {
        const double wf = 2.0 * PI_D * T->fcoarse[f] / 8000.0, cr = cos(wf * 79.5), ci = sin(wf * 79.5);
        for (int r = 0; r < RD_NQ; r++) {
            double ar = 0.0, ai = 0.0;
            for (int m = 0; m < RD_M; m++) { ar += q[r][m] * cos(wf * ((double)m - 79.5)); ai += q[r][m] * sin(wf * ((double)m - 79.5)); }
            b->alr[r][f] = ar * cr - ai * ci; b->ali[r][f] = ar * ci + ai * cr;
        }
    }
}
static int corrq_at(const void *ctx, int n, int k, double *v)
{
    const table_ctx *t = ctx;
    const int r = n >> 1, cp = n & 1, m = k >> 1, c = k & 1;
    const double sr = (double)t->T->p[m][0] * t->b->q[r][m], si = (double)t->T->p[m][1] * t->b->q[r][m];
    *v = cp == 0 ? (c == 0 ? sr : si) : (c == 0 ? si : -sr);
    return 0;
}
static int corra_at(const void *ctx, int n, int k, double *v)
{
    const table_ctx *t = ctx;
    const int f = n >> 1, cpp = n & 1, g = k >> 3, j = k & 7, np_ = j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4), r = np_ >> 1, cp = np_ & 1;
    const double ar = t->b->alr[r][f], ai = t->b->ali[r][f];
    *v = cpp == 0 ? (cp == 0 ? ar : -ai) : (cp == 0 ? ai : ar);
    return 0;
}
void rd_corrq16_fill(const rd_tables *T, const rd_corr_basis *b, unsigned short *out) { table_fill(T, b, 2 * RD_NQ, 2 * RD_M, corrq_at, 4096.0, out); }
void rd_corra16_fill(const rd_tables *T, const rd_corr_basis *b, unsigned short *out) { table_fill(T, b, 2 * RD_NFC, 2 * RD_NQ, corra_at, 1024.0, out); }
/* the two tables multiplied back together on the host, out[m][f] (re, im) ~ p_w[m][f]: max |difference| is returned */
double rd_corr_basis_check(const rd_tables *T, const rd_corr_basis *b)
{
    double worst = 0.0;
    for (int m = 0; m < RD_M; m++)
        for (int f = 0; f < RD_NFC; f++) {
            double re = 0.0, im = 0.0;
            for (int r = 0; r < RD_NQ; r++) {
                const double sr = (double)T->p[m][0] * b->q[r][m], si = (double)T->p[m][1] * b->q[r][m];
                re += b->alr[r][f] * sr - b->ali[r][f] * si; im += b->alr[r][f] * si + b->ali[r][f] * sr;
            }
            const double d = hypot(re - (double)T->p_w[m][f][0], im - (double)T->p_w[m][f][1]);
            if (d > worst) worst = d;
        }
    return worst;
}
/* the entry points of rade_host.h, each with a basis of its own on the stack (30 KB); an engine computes one per open and calls the functions above */
void rd_corrq16_table_fill(const rd_tables *T, unsigned short *out) { rd_corr_basis b; rd_corr_basis_fill(T, &b); rd_corrq16_fill(T, &b, out); }
void rd_corra16_table_fill(const rd_tables *T, unsigned short *out) { rd_corr_basis b; rd_corr_basis_fill(T, &b); rd_corra16_fill(T, &b, out); }
double rd_corr_tables_check(const rd_tables *T) { rd_corr_basis b; rd_corr_basis_fill(T, &b); return rd_corr_basis_check(T, &b); }      /* test aid (tests/test_host_cpu.py) */

/* The demodulator DFT of k_rx_sync2 on the f16 matrix cores (receiver_one, dsp.py:487-526: sym[s][c] = sum_n x_s[n] Wfwd[n][c]).  With the row
 * R[c][2n + comp] = (wr, -wi)[comp] the real part is R . (xr, xi) and the imaginary part R . (xi, -xr): ONE 32-row operand (30 carriers; rows 30, 31 are zero) serves
 * both, the two variants of the window are two groups of B columns.  2^12-scaled, [2 tiles][10 k-steps] like the pilot table above. */
static int wfwd_at(const void *ctx, int c, int k, double *v)
{
    const table_ctx *t = ctx;
    *v = (k & 1) == 0 ? t->T->Wfwd[k >> 1][c][0] : -t->T->Wfwd[k >> 1][c][1];
    return 0;
}
void rd_wfwd16_table_fill(const rd_tables *T, unsigned short *out) { table_fill(T, NULL, RD_NC, 2 * RD_M, wfwd_at, 4096.0, out); }

/* complex_bpf's 101 real taps (dsp.py:46-49) as the A operands of the matrix-core FIR (rade_bpf_fir.h: bpf_fir_tile): the Toeplitz rows
 * T[r][m] = 2^10 h[m - r] (0 outside 0 <= m - r <= 100), r = 0..15 outputs of a group, m = 0..127 window positions: [1 tile][4 k-steps] */
static int bpf_at(const void *ctx, int r, int m, double *v)
{
    const table_ctx *t = ctx;
    *v = (m - r >= 0 && m - r < RD_NTAP) ? t->T->bpf_h[m - r] : 0.0f;
    return 0;
}
void rd_bpf16_table_fill(const rd_tables *T, unsigned short *out) { table_fill(T, NULL, 16, 128, bpf_at, 1024.0, out); }
