// rade_rate.hip -- the rational sample-rate converter of rade_batch_rate_convert (include/rade_batch.h states the arithmetic): 48 / 44.1 kHz <-> 8 kHz, what `sox -r 8000`
// does in front of int16tof32.py in every off-air pipeline of the reference (radae_rx.sh:33,39).
//   k_rate_convert<FMT>   one workgroup per (tiles of a.tile consecutive outputs, stream); a workgroup walks its stream's tiles blockIdx.x, + gridDim.x, ...
// Output n sits at input position n M / L: i = floor(n M / L), ph = (n M) mod L, 64-bit integers, formed once per tile for its first output and from there in 32 bits
// (ph_a + o M < 2^24).  An output depends on (L, M, n) and the input alone: no state, and the same bits however a stream is cut into calls, tiles or threads (every output
// is one thread's sum over j = 0..T-1 in that order, one float32 accumulator per component, fused multiply-adds).
// LDS (dynamic, at most 80 KB: two workgroups per CU):
//   the table   once per workgroup, rows T + 1 floats apart.  T is a multiple of 32, so rows T apart would put tap j of EVERY row on one bank; one float more puts the
//               rows of the lanes of a wavefront on banks ph mod 32 (ds_read_b32: bank = dword address mod 32, conflicts among the 32 lanes of a half): conflict-free
//               for L <= 32 (6 / 1, 3 / 2), pseudo-random for the large L of 80 / 441 and 441 / 80.  L = 1: every lane reads the same word (a broadcast).
//   the window  the tile's input samples, zeros where the window leaves [in_base, in_base + n_in), converted from int16 on the way in; the real part and the imaginary
//               part in planes of their own (the real format has no second plane), read as single floats.
//               L = 1 (decimation by M): lane o reads sample o M + j, a stride of M floats: 2-way conflicts for M = 2 and 6, 4-way for 4, 8-way for 8, and padding
//               one float per 32 (or per 32 M) leaves single 2-way pairs, which cost the same LDS cycles.  So the window is stored DE-INTERLEAVED by k mod M: sample k at
//               (k mod M) P + k / M, P = ceil(len / M).  Tap j of every lane then comes from plane j mod M at consecutive words o + j / M: conflict-free for every M and
//               j, and the plane / word of a tap is the same for all lanes (scalar bookkeeping).
//               L > 1: sample k at word k.  Up-sampling lanes read the same or neighbouring samples (broadcasts and consecutive words); for 2 / 3 and 80 / 441 the lanes
//               advance by 1..2 and 5..6 words, an irregular stride with occasional 2-way pairs.
// None of this has been measured with the LDS conflict counter; DESIGN.md says so, and tools/time_rate.py gives the times.
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"

#define RATE_WG 256
#define RATE_LDS_MAX ((RD_RATE_TABLE_MAX + RD_RATE_TABLE_MAX / 32 + 2 * RD_RATE_WIN) * 4)      // L (T + 1) <= L T + L T / 32 floats
static_assert(RATE_LDS_MAX <= 80 * 1024, "table + window: two workgroups per CU");
static_assert((RD_RATE_WIN - 32 * RD_RATE_KMAX - RD_RATE_KMAX) / RD_RATE_KMAX + 1 >= 64, "a tile of at least 64 outputs at the steepest ratio");
static_assert((long long)RD_RATE_TILE_MAX * (RD_RATE_TABLE_MAX / 32) * RD_RATE_KMAX < (1 << 24), "ph_a + o M in 32 bits: o < the tile, M <= K L, L <= the table / 32");

// FMT: 0 complex64, 1 one int16 per sample (imaginary part +0, not computed), 2 two int16 per sample; the int16 operand is gain * (float)s, one float32 multiply
template <int FMT> __global__ __launch_bounds__(RATE_WG) void k_rate_convert(rd_rate_args a)
{
    extern __shared__ __attribute__((aligned(16))) float rate_lds[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const rd_rate_stream S = a.ps[b];
    const int L = a.L, M = a.M, T = a.T, pitch = a.T + 1;
    const int n_tiles = (S.n_out + a.tile - 1) / a.tile;
    if ((int)blockIdx.x >= n_tiles) return;
    float *C = rate_lds, *wre = rate_lds + L * pitch, *wim = wre + RD_RATE_WIN;          // wim: not there (and not touched) in the real format
    const float2 *xc = (const float2 *)a.x + (size_t)b * a.x_stride;
    const short *xs = (const short *)a.x + (size_t)b * a.x_stride;
    float2 *y = (float2 *)a.y + (size_t)b * a.y_stride;
    const float gain = a.gain;
    for (int i = tid; i < L * T; i += RATE_WG) { const int r = i / T; C[r * pitch + (i - r * T)] = a.taps[i]; }
    const int D = L == 1 ? M : 1;                                                        // planes of the window
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int o0 = tile * a.tile, cnt = min(a.tile, S.n_out - o0);
        const long long pos_a = (S.n0 + o0) * (long long)M;                              // <= 2^62: checked by the entry
        const long long i_a = pos_a / L;
        const unsigned ph_a = (unsigned)(pos_a - i_a * L);
        const long long i_lo = i_a - (T / 2 - 1);                                        // first sample of the tile's window
        const int len = min((int)((ph_a + (unsigned)(cnt - 1) * (unsigned)M) / (unsigned)L) + T, RD_RATE_WIN - (D - 1));
        const int P = (len + D - 1) / D;                                                 // D P <= len + D - 1 <= RD_RATE_WIN
        __syncthreads();                                                                 // the table is there; the previous tile's window has been read
        {
            int q = tid / D, r = tid - q * D;                                            // k = q D + r, advanced by RATE_WG without further divisions
            const int dq = RATE_WG / D, dr = RATE_WG - dq * D;
            for (int k = tid; k < len; k += RATE_WG) {
                const long long g = i_lo + k - S.in_base;                                // index into the stream's row: read inside [0, n_in) only
                const bool in = g >= 0 && g < S.n_in;
                const int w = r * P + q;
                if (FMT == 0) { const float2 v = in ? xc[g] : make_float2(0.0f, 0.0f); wre[w] = v.x; wim[w] = v.y; }
                else if (FMT == 1) wre[w] = in ? gain * (float)xs[g] : 0.0f;
                else { wre[w] = in ? gain * (float)xs[2 * g] : 0.0f; wim[w] = in ? gain * (float)xs[2 * g + 1] : 0.0f; }
                q += dq; r += dr; if (r >= D) { r -= D; q++; }
            }
        }
        __syncthreads();
        for (int o = tid; o < cnt; o += RATE_WG) {
            const unsigned v = ph_a + (unsigned)o * (unsigned)M;
            const unsigned w = v / (unsigned)L;                                          // x[i - (T / 2 - 1)] is sample w of the window
            const float *row = C + (v - w * (unsigned)L) * pitch;
            float re = 0.0f, im = 0.0f;
            if (D == 1) {
                const float *pr = wre + w, *pi = wim + w;
#pragma unroll 8
                for (int j = 0; j < T; j++) {
                    const float c = row[j];
                    re = fmaf(c, pr[j], re);
                    if (FMT != 1) im = fmaf(c, pi[j], im);
                }
            } else {                                                                     // L = 1: ph = 0, w = o M; tap j reads plane j mod M at word o + j / M
                int base = (int)(w / (unsigned)M), r = 0;
                for (int j = 0; j < T; j++) {
                    const float c = row[j];
                    re = fmaf(c, wre[r * P + base], re);
                    if (FMT != 1) im = fmaf(c, wim[r * P + base], im);
                    if (++r == M) { r = 0; base++; }
                }
            }
            y[o0 + o] = make_float2(re, im);                                             // one 8-byte store per sample: any y_stride, any parity of n_out
        }
    }
}

template <int FMT> static int rate_launch(const rd_rate_args *a, dim3 grid, size_t lds, hipStream_t s)
{
    rd_dyn_lds_once<k_rate_convert<FMT>, RATE_LDS_MAX>();
    hipLaunchKernelGGL(k_rate_convert<FMT>, grid, dim3(RATE_WG), lds, s, *a);
    return (int)hipGetLastError();
}

extern "C" int rd_launch_rate_convert(const rd_rate_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_out <= 0) return 0;
    if (a->L < 1 || a->M < 1 || a->T != 32 * ((a->M + a->L - 1) / a->L) || a->T > 32 * RD_RATE_KMAX || a->L * a->T > RD_RATE_TABLE_MAX) return -1;
    if (a->tile != rd_rate_tile(a->L, a->M, a->T)) return -1;
    const int n_tiles = (a->max_out + a->tile - 1) / a->tile;
    int gx = 2048 / a->B; if (gx < 1) gx = 1;                                            // about 2048 workgroups per launch: the table is loaded once per workgroup, not per tile
    if (gx > n_tiles) gx = n_tiles;
    const size_t lds = sizeof(float) * ((size_t)a->L * (a->T + 1) + (a->fmt == 1 ? 1 : 2) * RD_RATE_WIN);
    const dim3 grid(gx, a->B);
    if (a->fmt == 0) return rate_launch<0>(a, grid, lds, (hipStream_t)s);
    if (a->fmt == 1) return rate_launch<1>(a, grid, lds, (hipStream_t)s);
    if (a->fmt == 2) return rate_launch<2>(a, grid, lds, (hipStream_t)s);
    return -1;
}
