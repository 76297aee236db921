// rade_rx.hip -- THE receiver of the RADE hot path: do_radae_rx (radae_rxe.py:171-330) for one stream per workgroup, all of its calls in one launch.
//
//   k_bpf_chain / k_bpf_fir / k_bpf_advance   complex_bpf.bpf (dsp.py:63-102) for every sample of a rade_batch_rx invocation, ahead of the receiver kernel
//                 (round 4: the band-pass filter does not depend on any sync decision, so it left the per-stream serial chain)
//   k_rx_sync2    acquisition (detect_pilots / refine / check_pilots, dsp.py:178-320), sync state machine, frequency correction, OFDM demod +
//                 3-pilot LS EQ (dsp.py:418-526), the CoreDecoder stage (radae_base.py:358-430) and UW accounting (rade_api.c:480-513): 256 threads
//                 and at most 80 KB of LDS per stream, so that two streams share a CU
//   k_batch_reset radae_rxe.py:128-142 (and the encoder / decoder start-of-utterance state, one launch)
//
// ONE translation unit, one file per stage, included below in the order the stages need each other: rade_rx_dec.h (decoder stage), rade_rx_search.h (pilot
// search over rade_corr2.h, the correlator it shares with check_pilots and rade_acq.hip; workgroup reductions), rade_rx_refine.h, rade_rx_check.h, rade_bpf.h (band-pass arithmetic).  This file keeps the per-stream state (RxScalars,
// RxShared2), the developer switches, the decoder hand-over, the kernels and their launch shims.  The band-pass kernels stay in this unit: in a unit of
// their own they compile to the same code, but k_rx_sync2, left as the only caller of the shared band-pass functions here, does not (tools/codegen_diff.py).
// Rounds 2-3 carried a second receiver kernel (512 threads, one stream per CU) that this one was forked from; it is gone: one receiver, every fix lands once.
#include "rade_devutil.h"
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

enum { ST_SEARCH = 0, ST_CANDIDATE = 1, ST_SYNC = 2 };
struct RxScalars {
    int state, nin, tmax, tmax_candidate, valid_count, uw_errors, synced_count, mf, f_ind_max, dec_reset_pending, has_eoo;
    uint32_t lcg;
    unsigned rxmax_cur, rxmax_h0, rxmax_h1;   // float bits of max |re|,|im| of the filtered samples of this call / the two calls before (check_pilots operand scale)
    int consumed_inv, calls_inv, valid_inv, eoo_inv, n_calls, n_rows, uw_from_row, consumed_round, pending_valid, out_base;
    int tab_ok;               // refine()'s per-frequency constants for the CURRENT fmax are in LDS (left by the previous synchronised call's idle wavefront)
    int bpf_grid, nin0;       // the stream's calls still follow the block grid of the invocation's band-pass pre-pass (k_bpf_fir); the grid's first block length
    int entry;                // this candidate call enters sync (decided by thread 0 before a barrier: see do_entry)
    int go, need_decode, batch_call0, state_before, nin_before, valid_output, endofover, uw_fail, candidate, dt_valid, dt_new, lds_sync;
    float snr_est, mag; float2 bpf_phase;
    double fmax, foff_err, rph_r, rph_i, Dthresh, Dtmax12, Dtmax12_eoo;
    double rph_th;                        // k_rx_sync2: the phase accumulator as an angle in [-pi, pi] (rph_r + j rph_i = e^{j rph_th})
};

__device__ static constexpr uint32_t LCG_A[48] = { 1664525u, 389569705u, 2940799637u, 158984081u, 2862450781u, 3211393721u, 1851289957u, 3934847009u, 2184914861u, 246739401u, 1948736821u, 2941245873u, 4195587069u, 4088025561u, 980655621u, 2001863745u, 657792333u, 65284841u, 1282409429u, 3808694225u, 2968195997u, 2417331449u, 2878627493u, 307989601u, 504219373u, 1897564169u, 2574089845u, 3294562801u, 3478292285u, 2651335705u, 2523738949u, 666245249u, 4137395341u, 2604435753u, 1706708245u, 3963176977u, 3678957277u, 3530469177u, 3858799589u, 629287073u, 3146069549u, 3820924489u, 2403397557u, 2390444593u, 2593868413u, 4291139161u, 1705056389u, 3186638017u };
__device__ static constexpr uint32_t LCG_C[48] = { 1013904223u, 1196435762u, 3519870697u, 2868466484u, 1649599747u, 2670642822u, 1476291629u, 2748932008u, 2180890343u, 2498801434u, 3421909937u, 3167820124u, 2636375307u, 3801544430u, 28987765u, 2210837584u, 3039689583u, 1338634754u, 1649346937u, 2768872580u, 2254235155u, 2326606934u, 1719328701u, 1061592568u, 53332215u, 1140036074u, 4224358465u, 2629538988u, 1946028059u, 573775550u, 1473591045u, 95141024u, 1592739711u, 1618554578u, 4257218569u, 2685635028u, 2617994019u, 740185638u, 4194465613u, 2426187848u, 967350023u, 366635194u, 2557108433u, 3503432700u, 353185579u, 706247310u, 408928405u, 1855199472u };

#define NT2 256
#define NW2 (NT2 / 64)
// thread index rebuilt from the lane counter and the wavefront's index (held in a scalar register): three instructions wherever it
// is needed, instead of one value that stays live -- and gets spilled -- across the whole receive call (rx_tid() keeps threadIdx.x
// alive the same way).  RX2_SYNC: a barrier of k_rx_sync2's call loop with `tid` rebuilt behind it, so that no live range of it crosses a barrier
__device__ __forceinline__ int rx2_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ int rx2_tid(int wv) { int l = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); asm volatile("" : "+v"(l)); return (wv << 6) | l; }
#define RX2_SYNC() do { __syncthreads(); tid = rx2_tid(wv); } while (0)
// developer aid (-DRX2_CENSUS, tools/rx2_census.sh): a.variant >> 8 is a mask that skips the decoder stage / its recurrence or runs an idempotent
// phase twice, so that the per-phase share of the instruction counters (rocprofv3 --pmc SQ_INSTS_*) is the difference between two runs
#ifdef RX2_CENSUS
#define CENSUS(bit) ((a.variant >> 8) & (bit))
#define CENSUS_REPS(bit) (CENSUS(bit) ? 2 : 1)
#else
#define CENSUS(bit) 0
#define CENSUS_REPS(bit) 1
#endif
#ifdef RD_PHASE_TIMING   // developer aid: per-phase shader-clock totals of workgroup 0 (tools/ab_build.sh timing -DRD_PHASE_TIMING; tools/phase_timing2.py)
__device__ long long g_phase_cycles2[32];
#define PH2_T0() long long ph2_t_ = clock64()
#define PH2(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { long long n_ = clock64(); atomicAdd((unsigned long long *)&g_phase_cycles2[i], (unsigned long long)(n_ - ph2_t_)); ph2_t_ = n_; } } while (0)
#define PH2_RESTART() do { ph2_t_ = clock64(); } while (0)
extern "C" void rd_debug_phase_cycles2(long long *out) { hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_cycles2), sizeof(long long) * 32); long long z[32] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles2), z, sizeof z); }
#else
#define PH2_T0() do { } while (0)
#define PH2(i) do { } while (0)
#define PH2_RESTART() do { } while (0)
#endif
#include "rade_rx_dec.h"

// ---- LDS of k_rx_sync2: at most 80 KB, so that two workgroups share a CU ----
struct RxShared2 {
    RxScalars S;
    float rx_unsc; int lcg_next;   // a synchronised call's operand un-scale (rx2_operand_scale) and next LCG state, from the planes phase to check_pilots / the demodulator / thread 0
    double2 rq[4], rzc, rph[24], rrot[24]; double ral[24];   // refine(), in-sync grid: e^{-jw_c 40 q}, e^{-jw_c}, e^{-j(w_k - w_c) 79.5}, e^{-jw_k Nmf}, (w_k - w_c) 80
    int rows48[48];
    double redd[(NW2 + 1) * 10];
    float redf[16]; int redi[16]; int redj[16];
    double corrp[NW2][8];
    union {
      struct {
        float2 rxb[RD_RXBUF];                                   // rx_buf (radae_rxe.py:141): parked in the stream's HBM record while the decoder stage runs
        float rowsum1[RD_NMF], rowsum2[RD_NMF];                 // likewise
        union {
          struct {                                              // BPF / synchronised state
            __attribute__((aligned(16))) float2 xm[1408];       // BPF [mem | mixed-down new]; refine(): rx window as doubles; rx1[1152] for the demodulator
            double2 pd[RD_M], pendd[RD_M];                      // pilot / end-of-over replicas as doubles (reloaded with the state: S.lds_sync)
            float2 sym[6][RD_NC]; float2 rp[2][RD_NC];
            float eqP[RD_NC]; float2 eqPmat[RD_NC][2][3], eqrot[RD_NC]; float eq_pg, eq_snrc1, eq_snrc2, eq_pad;
            float2 cisA[2][18], cisB[2][64];                    // the frequency-corrected window's phasor e^{j(theta - w (n + 1))} = cisA[n >> 6] cisB[n & 63], one copy per wavefront that cuts the window
            union {
              struct {
                u32x2 rxhl[RD_RXBUF];                           // check_pilots: rx_buf in two binary16 planes, a sample's (high, low) words side by side: one 8-byte read brings both
                double rmom[2][2][64][4];                       // refine(), in-sync grid: partial moment tiles [half of the samples][frame]
                double mtot[2][16][16];                         // the moments [frame][2 m + (re | im)][t]
              };
              struct {                                          // refine() on sync entry (+-10 Hz): direct sums
                double2 rtw[80], rrot80[80], rt80[80];
                float2 dtr[2 * 80 * 16];
              };
            };
          };
          struct {                                              // search / candidate state: two-stage pilot correlator on the matrix cores (rx2_detect_q)
            __attribute__((aligned(16))) _Float16 sA[2][2 * 2 * 2 * 64 * 8];   // stage 1's A operands (moment table) of TWO k-steps, double-buffered (2 x 8 KB)
            __attribute__((aligned(16))) _Float16 sA2[5 * 2 * 64 * 8];         // stage 2's A operands (moments -> 40 frequencies), whole: 10 KB
            unsigned srxh[RD_RXBUF], srxl[RD_RXBUF];            // rx_buf in two binary16 planes
          };
        };
      };
      __attribute__((aligned(16))) unsigned char dec_raw[sizeof(DecShared2)];
    };
};
static_assert(sizeof(RxShared2) <= 80 * 1024, "two k_rx_sync2 workgroups must fit the 160 KiB LDS of a CU");

#include "rade_rx_search.h"
#include "rade_rx_refine.h"

// rx_buf and the |Dt| row sums from the stream's HBM record into LDS: every load of a thread requested before the first store (as a plain loop
// the compiler cannot tell that the LDS stores do not alias the record and waits for each load before the next: 13 round trips in a row)
__device__ __forceinline__ void rx2_load_rxbuf(RxShared2 *sh, const rd_rx_stream *st, int tid)
{
    constexpr int NB_ = (RD_RXBUF + NT2 - 1) / NT2, NR_ = (RD_NMF + NT2 - 1) / NT2;
    float2 v[NB_]; float r1[NR_], r2[NR_];
#pragma unroll
    for (int q = 0; q < NB_; q++) { const int i = min(tid + q * NT2, RD_RXBUF - 1); v[q] = make_float2(st->rx_buf[i][0], st->rx_buf[i][1]); }
#pragma unroll
    for (int q = 0; q < NR_; q++) { const int i = min(tid + q * NT2, RD_NMF - 1); r1[q] = st->rowsum1[i]; r2[q] = st->rowsum2[i]; }
#pragma unroll
    for (int q = 0; q < NB_; q++) { const int i = tid + q * NT2; if (i < RD_RXBUF) sh->rxb[i] = v[q]; }
#pragma unroll
    for (int q = 0; q < NR_; q++) { const int i = tid + q * NT2; if (i < RD_NMF) { sh->rowsum1[i] = r1[q]; sh->rowsum2[i] = r2[q]; } }
}

// ---- decoder + output stage for the rows a stream has pending (four wavefronts, chunks of 12 rows) -----------
// rx_buf and the row sums leave LDS for the duration (the stage's 64 KB overlay them): out to the stream's HBM record, back afterwards
__device__ __forceinline__ void rx2_decode_pending(RxShared2 *sh, const rd_sync_args &a, int b)
{
    RxScalars *S = &sh->S;
    DecShared2 *ds = (DecShared2 *)&sh->dec_raw[0];
    rd_rx_round *rnd = a.round + b;
    rd_rx_stream *st = a.st + b;
    const int tid = rx_tid();
    const int Tb = S->n_rows;
    PH2_T0();
    for (int i = tid; i < RD_RXBUF; i += NT2) { st->rx_buf[i][0] = sh->rxb[i].x; st->rx_buf[i][1] = sh->rxb[i].y; }
    for (int i = tid; i < RD_NMF; i += NT2) { st->rowsum1[i] = sh->rowsum1[i]; st->rowsum2[i] = sh->rowsum2[i]; }
    __syncthreads();
    PH2(19);
    for (int i = tid; i < Tb; i += NT2) ds->rst[i] = rnd->row_reset[i];
    if (tid == 0) S->lds_sync = 0;
    __syncthreads();
    for (int c0 = 0; c0 < Tb; c0 += DQ2_ROWS) {
        const int n = min(DQ2_ROWS, Tb - c0);
        unsigned rstmask = 0u;
        for (int t = 0; t < n; t++) rstmask |= ds->rst[c0 + t] ? (1u << t) : 0u;
        if (!CENSUS(1)) dq2_layers(ds, a.dec, b, a.dec.z + (size_t)b * a.dec.z_sb + (size_t)c0 * RD_LATENT, a.dec.out + (size_t)b * a.dec.out_sb + (size_t)c0 * a.dec.out_w, n, rstmask, CENSUS(2));
    }
    const float *f84 = a.dec.out + (size_t)b * a.dec.out_sb;
    for (int r = tid; r < Tb; r += NT2) ds->err[r] = f84[r * RM_FEAT_AUX + RM_NFEAT] > 0.0f ? 1 : 0;
    float *out = a.features_out + (size_t)b * a.feat_stride + (size_t)S->out_base * RD_FEAT_MF;
    for (int i0 = tid; i0 < (Tb / 3) * RD_FEAT_MF; i0 += 4 * NT2) {      // four loads in flight per thread (a plain loop waits for each load before its store: the stores may alias)
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = min(i0 + q * NT2, (Tb / 3) * RD_FEAT_MF - 1), fr = i / RM_FILE_FRAME, j = i - fr * RM_FILE_FRAME;
            const int row = fr >> 2, sub = fr & 3;
            v[q] = f84[row * RM_FEAT_AUX + sub * (RM_NFEAT + 1) + min(j, RM_NFEAT - 1)];
            if (j >= RM_NFEAT) v[q] = 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) { const int i = i0 + q * NT2; if (i < (Tb / 3) * RD_FEAT_MF) out[i] = v[q]; }
    }
    __syncthreads();
    if (a.trace) {
        for (int c = S->batch_call0 + tid; c < S->n_calls; c += NT2) {
            const int idx = rnd->call_trace_idx[c];
            if (idx >= a.trace_cap) continue;
            int e = 0;
            for (int r = rnd->call_row_lo[c]; r < rnd->call_row_hi[c]; r++) e += ds->err[r];
            a.trace[(size_t)b * a.trace_cap + idx].uw_errors += e;
        }
    }
    if (tid == 0) {
        int add = 0;
        for (int r = S->uw_from_row; r < Tb; r++) add += ds->err[r];
        S->uw_errors += add;
        S->out_base += Tb / 3; S->n_rows = 0; S->uw_from_row = 0; S->pending_valid = 0; S->batch_call0 = S->n_calls; S->need_decode = 0;
    }
    __syncthreads();
    PH2_RESTART();
    rx2_load_rxbuf(sh, st, tid);
    __syncthreads();
    PH2(19);
}

// radae_rxe.py --bypass_dec (:300-302, :315; the mode rade_api.c drives with the external C decoder): the pending z_hat rows leave as they are -- 240 floats per
// valid modem frame -- and the aux-bit (UW) errors are never summed, so uw_fail cannot occur (sum_uw_errors is only called behind the decoder, :303-312)
__device__ __forceinline__ void rx2_bypass_pending(RxShared2 *sh, const rd_sync_args &a, int b)
{
    RxScalars *S = &sh->S;
    const int tid = rx_tid();
    const int Tb = S->n_rows;
    const float *z = a.dec.z + (size_t)b * a.dec.z_sb;
    float *out = a.features_out + (size_t)b * a.feat_stride + (size_t)S->out_base * RD_ZMF;
    for (int i = tid; i < Tb * RD_LATENT; i += NT2) out[i] = z[i];
    __syncthreads();
    if (tid == 0) { S->out_base += Tb / 3; S->n_rows = 0; S->uw_from_row = 0; S->pending_valid = 0; S->batch_call0 = S->n_calls; S->need_decode = 0; }
    __syncthreads();
}

#include "rade_rx_check.h"
#include "rade_bpf.h"

#ifndef RX2_WG_PER_CU
#define RX2_WG_PER_CU 2          /* developer switch: the register budget of a build that would hold three workgroups per CU (168 VGPRs) */
#endif
__global__ __launch_bounds__(NT2, RX2_WG_PER_CU) void k_rx_sync2(rd_sync_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    RxShared2 *sh = (RxShared2 *)smem_raw;
    RxScalars *S = &sh->S;
    const rd_tables *tab = a.tab;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int wv = rx2_wave();
    rd_rx_stream *st = a.st + b;
    rd_rx_round *rnd = a.round + b;
    const float2 *rxin = (const float2 *)a.rx + (size_t)b * a.rx_stride;

    // ---- load the stream's working set into LDS
    rx2_load_rxbuf(sh, st, tid);
    if (tid == 0) {
        S->state = st->state; S->nin = st->nin; S->tmax = st->tmax; S->tmax_candidate = st->tmax_candidate; S->valid_count = st->valid_count;
        S->uw_errors = st->uw_errors; S->synced_count = st->synced_count; S->mf = st->mf; S->f_ind_max = st->f_ind_max;
        S->dec_reset_pending = st->dec_reset_pending; S->has_eoo = st->has_eoo; S->lcg = st->lcg;
        S->rxmax_cur = st->rxmax[0]; S->rxmax_h0 = st->rxmax[1]; S->rxmax_h1 = st->rxmax[2];
        S->fmax = st->fmax; S->foff_err = st->foff_err; S->rph_th = st->rx_theta;     // rx_phase (radae_rxe.py:227-233) kept as its angle: see the corrected window
        S->Dthresh = st->Dthresh; S->Dtmax12 = st->Dtmax12; S->Dtmax12_eoo = st->Dtmax12_eoo; S->snr_est = st->snr_est;
        S->bpf_phase = make_float2(st->bpf.phase[0], st->bpf.phase[1]);      // only used off the grid (rx2_bpf_own)
        S->consumed_inv = a.acc[b * 4 + 0]; S->calls_inv = a.acc[b * 4 + 1]; S->valid_inv = a.acc[b * 4 + 2]; S->eoo_inv = a.acc[b * 4 + 3];
        S->n_calls = 0; S->n_rows = 0; S->uw_from_row = 0; S->consumed_round = 0; S->pending_valid = 0; S->out_base = S->valid_inv;
        S->go = 0; S->dt_valid = st->dt_valid; S->dt_new = 0; S->lds_sync = 0; S->need_decode = 0; S->batch_call0 = 0; S->tab_ok = 0;
        S->bpf_grid = st->bpf.grid_off == 0; S->nin0 = __float_as_int(((const float *)a.bpf_chain)[(size_t)b * a.chain_stride * 2]);
    }
    const int avail = a.avail[b];
    const long long wg_t0 = clock64();
    __syncthreads();
    PH2_T0(); PH2(0);

    for (int it = 0; it <= a.round_calls; it++) {
        int tid = rx2_tid(wv);
        auto prepare_next = [&]() {
            const int calls_inv = S->calls_inv, n_calls = S->n_calls, valid_inv = S->valid_inv, consumed = S->consumed_inv, nin_n = S->nin;
            const int n_rows = S->n_rows, st_n = S->state, sc = S->synced_count;
            const unsigned m0 = S->rxmax_h0, m1 = S->rxmax_cur, m2 = S->rxmax_h1;
            const int go = (int)(calls_inv < a.max_calls) & (int)(n_calls < a.round_calls) & (int)(valid_inv < a.feat_cap) & (int)(consumed + nin_n <= avail);
            const int need = (int)(n_rows > 0) & ((go ^ 1) | ((int)(st_n == ST_SYNC) & (int)(((sc + 1) % 8) == 0)) | (int)(n_rows + 3 > a.dec_rows));
            S->need_decode = need; S->go = go;
            S->rxmax_h1 = go ? m0 : m2; S->rxmax_h0 = go ? m1 : m0; S->rxmax_cur = go ? 0u : m1;
            S->state_before = st_n; S->nin_before = nin_n;
            S->valid_output = 0; S->endofover = 0; S->uw_fail = 0; S->candidate = 0;
        };
        if (it == 0) {
            if (tid == 0) prepare_next();
            RX2_SYNC();
        }
        PH2(1);
        if (S->need_decode) { if (a.bypass_dec) rx2_bypass_pending(sh, a, b); else rx2_decode_pending(sh, a, b); PH2(2); }
        if (!S->go) break;
        const int nin = S->nin, state = S->state;
        if (tid == 0 && state != ST_SYNC) S->tab_ok = 0;
        const int mf0 = S->mf, n_rows0 = S->n_rows;
        auto state_update = [&](int entry, int valid_out, int eoo) {
            int next_state = state;
            if (state == ST_SEARCH) {
                if (S->candidate) { next_state = ST_CANDIDATE; S->tmax_candidate = S->tmax; S->valid_count = 1; }
            } else if (state == ST_CANDIDATE) {
                if (entry) {
                    next_state = ST_SYNC;
                    S->dec_reset_pending = 1; S->synced_count = 0; S->uw_fail = 0; S->uw_errors = 0; S->uw_from_row = S->n_rows; S->valid_count = 25;
                } else if (S->candidate && abs(S->tmax - S->tmax_candidate) < RD_NCP) S->valid_count++;
                else next_state = ST_SEARCH;
            } else {
                const bool unsync_enable = !(a.unsync_off_after >= 0 && S->synced_count > a.unsync_off_after);
                if (S->candidate) S->valid_count = 25;
                else { S->valid_count--; if (unsync_enable && S->valid_count == 0) next_state = ST_SEARCH; }
                if (unsync_enable && (eoo || S->uw_fail)) next_state = ST_SEARCH;
            }
            S->dt_valid = (state != ST_SYNC && next_state != ST_SYNC) ? S->dt_new + 1 : 0;
            S->state = next_state;
            if (next_state == ST_SEARCH) S->nin = RD_NMF;
            S->mf++;
            const int ret = valid_out | (eoo << 1);
            const int call_idx = S->mf - 2;
            if (valid_out) {
                for (int k = 0; k < 3; k++) { const int rf = (k == 0) ? S->dec_reset_pending : 0; rnd->row_reset[S->n_rows + k] = rf; }
                S->dec_reset_pending = 0; S->n_rows += 3; S->pending_valid++; S->valid_inv++;
            }
            if (eoo) { S->has_eoo = 1; S->eoo_inv++; }
            const int nc = S->n_calls;
            rnd->call_ret[nc] = ret; rnd->call_row_lo[nc] = S->uw_from_row; rnd->call_row_hi[nc] = S->n_rows; rnd->call_trace_idx[nc] = call_idx;
            S->n_calls = nc + 1; S->calls_inv++;
        };
        const int cons0 = S->consumed_inv, calls0 = S->calls_inv;
        // ---- complex_bpf.bpf (dsp.py:63-102) ran ahead of this kernel for every sample of the invocation (k_bpf_fir): the filter does not depend on
        // any sync decision.  This call's nin filtered samples are rxf[cons0 ..) as long as the stream's calls follow the pre-pass's block grid (first
        // block = the nin the invocation started with, then Nmf each: the reference's own call partition unless nin changes inside an invocation);
        // after such a timing slip the stream filters the rest of the invocation's samples itself (rx2_bpf_own: same arithmetic, cold path).
        float2 *rxf = (float2 *)a.rxf + (size_t)b * a.rxf_stride;
        const bool on_grid = S->bpf_grid && nin == (calls0 ? RD_NMF : S->nin0);
        if (!on_grid) { rx2_bpf_own(sh, a, b, rxf, cons0, nin, calls0); tid = rx2_tid(wv); }
        constexpr int NNEW = (RD_NINMAX + NT2 - 1) / NT2;
        float2 nv[NNEW];
#pragma unroll
        for (int q = 0; q < NNEW; q++) { const int i = tid + q * NT2; nv[q] = i < nin ? (on_grid ? rxf[cons0 + i] : sh->xm[i]) : make_float2(0.0f, 0.0f); }
        if (state == ST_SYNC && !S->lds_sync) {      // pilot replicas and equaliser constants share LDS with the pilot search and the decoder stage
            // (after every decoder stage: all of a thread's table loads requested before its first LDS store -- as one statement after the other each load was waited for)
            const int i0 = min(tid, RD_M - 1), cc = min(tid, RD_NC - 1), c6 = min(tid, RD_NC * 6 - 1) / 6, r6 = min(tid, RD_NC * 6 - 1) - 6 * c6;
            const float2 vp = ld2(tab->p, i0), ve = ld2(tab->pend, i0);
            const float vP = tab->P[cc]; const float2 vr = ld2(tab->eq_rot, cc);
            const float2 vm_ = make_float2(tab->Pmat[c6][r6 / 3][r6 % 3][0], tab->Pmat[c6][r6 / 3][r6 % 3][1]);
            const float g0_ = tab->pilot_gain, g1_ = tab->snr_c1, g2_ = tab->snr_c2;
            if (tid < RD_M) { sh->pd[tid] = make_double2(vp.x, vp.y); sh->pendd[tid] = make_double2(ve.x, ve.y); }
            if (tid < RD_NC) { sh->eqP[tid] = vP; sh->eqrot[tid] = vr; }
            if (tid < RD_NC * 6) sh->eqPmat[c6][r6 / 3][r6 % 3] = vm_;
            if (tid == 0) { sh->eq_pg = g0_; sh->eq_snrc1 = g1_; sh->eq_snrc2 = g2_; }
        }
        PH2(3);
        // rx_buf shift and append (radae_rxe.py:196-197); the largest component of the new samples sets the operand scale of the binary16 planes
        constexpr int NK = (RD_RXBUF + NT2 - 1) / NT2;
        float2 keep[NK];
#pragma unroll
        for (int q = 0; q < NK; q++) { const int i = tid + q * NT2; keep[q] = (i + nin < RD_RXBUF) ? sh->rxb[i + nin] : make_float2(0.0f, 0.0f); }
        float mloc = 0.0f;
#pragma unroll
        for (int q = 0; q < NNEW; q++) mloc = fmaxf(mloc, fmaxf(fabsf(nv[q].x), fabsf(nv[q].y)));
        mloc = wave_max_f32(mloc);
        RX2_SYNC();
#pragma unroll
        for (int q = 0; q < NK; q++) { const int i = tid + q * NT2; if (i + nin < RD_RXBUF) sh->rxb[i] = keep[q]; }
#pragma unroll
        for (int q = 0; q < NNEW; q++) { const int i = tid + q * NT2; if (i < nin) sh->rxb[RD_RXBUF - nin + i] = nv[q]; }
        if ((tid & 63) == 0) atomicMax(&S->rxmax_cur, __float_as_uint(mloc));
        if (tid == 0) {
            if (state == ST_SYNC) S->lds_sync = 1;
            S->consumed_inv += nin; S->consumed_round += nin;
        }
        RX2_SYNC();

        PH2(5);
        if (state == ST_SEARCH || state == ST_CANDIDATE) {
            // ---- acquisition.detect_pilots (dsp.py:178-231) by FFT convolution, |Dt2| of the previous call reused as |Dt1|
            float best = -1.0f; int bt = 0x7fffffff, bfi = 0;
            const bool cached = S->dt_valid != 0;
            const int oldb = cached ? S->dt_valid - 1 : 0, newb = 1 - oldb;
            float *cache = a.dtcache + (size_t)b * 2 * RD_NFC * RD_NMF;
            if (tid == 0) { S->lds_sync = 0; S->dt_new = newb; }
            if (cached) {
                constexpr int NR = (RD_NMF + NT2 - 1) / NT2;
                float r2[NR];
#pragma unroll
                for (int q = 0; q < NR; q++) r2[q] = sh->rowsum2[min(tid + q * NT2, RD_NMF - 1)];
#pragma unroll
                for (int q = 0; q < NR; q++) sh->rowsum1[min(tid + q * NT2, RD_NMF - 1)] = r2[q];   // each thread moves its own slots: no barrier in between
            }
            RX2_SYNC();
            PH2(6);
            float rx_sc, rx_unsc;
            rx2_operand_scale(S, rx_sc, rx_unsc);
            for (int i = tid; i < RD_RXBUF; i += NT2) {      // operand planes of the whole rx_buf (as for check_pilots in the synchronised state)
                float2 v = sh->rxb[i]; v.x *= rx_sc; v.y *= rx_sc;
                rx2_split16(v, sh->srxh[i], sh->srxl[i]);
            }
            if (CENSUS(512)) { float b_ = -1.0f; int t_ = 0x7fffffff, f_ = 0; rx2_detect_q(sh, a.corrq16, a.corra16, cache, cached ? 1 : 0, oldb, newb, rx_unsc, b_, t_, f_); asm volatile("" :: "v"(b_), "v"(t_), "v"(f_)); }
            rx2_detect_q(sh, a.corrq16, a.corra16, cache, cached ? 1 : 0, oldb, newb, rx_unsc, best, bt, bfi);
            PH2(7);
            block_argmax2(sh, best, bt, bfi);
            const float Dmax = best; const int tbest = bt, fbest = bfi;
            const float sr = sigma_r_from_rowsums2(sh);
            if (tid == 0) {
                S->Dthresh = (double)(2.0f * sr) * RD_SQRT_NLOG_1EM5_5;
                if (Dmax > 0.0f) { S->tmax = tbest; S->f_ind_max = fbest; S->fmax = -50.0 + 2.5 * fbest; S->Dtmax12 = (double)Dmax; }
                else { S->tmax = 0; S->f_ind_max = 0; S->fmax = 0.0; S->Dtmax12 = 0.0; }
                S->candidate = S->Dtmax12 > S->Dthresh;
                S->entry = S->candidate && (abs(S->tmax - S->tmax_candidate) < RD_NCP) && (S->valid_count + 1 > 3);
            }
            RX2_SYNC();
        } else {
            // ---- in sync: refine, check_pilots, slips, UW, frequency correction, demod
            int tm_ref; double fm_ref;
            {
                const int tm = S->tmax; const double fm = S->fmax;
                const int t0 = max(0, tm - 8);
                int tnew = tm; double fhat = fm;
                {   // check_pilots' operand planes of the whole rx_buf
                    float rx_sc, rx_unsc;
                    rx2_operand_scale(S, rx_sc, rx_unsc);
                    if (tid == 0) sh->rx_unsc = rx_unsc;
                    if (tid >= NT2 - 64) {
                        // side jobs of the call on the fourth wavefront (they only depend on last call's results): the per-frequency constants of
                        // refine()'s grid, check_pilots' 48 row draws, and the first touch of the NEXT call's filtered samples (HBM + address translation:
                        // 256 streams read 256 separate regions; one load per 128-byte line, values dropped)
                        const int l = tid - (NT2 - 64);
                        if (!S->tab_ok) refine2_tables_sync(sh, l, fm - 1.0, fm + 1.0, 0.1);      // (first synchronised call after sync entry: nobody prepared them)
                        const int k = min(l, 47);
                        const uint32_t x = LCG_A[k] * S->lcg + LCG_C[k];
                        if (l < 48) sh->rows48[k] = (int)((x >> 8) % RD_NMF);
                        if (l == 47) sh->lcg_next = (int)x;
                        const int rem = min(avail - cons0 - nin, RD_NINMAX);
                        float t = 0.0f;
#pragma unroll
                        for (int q = 0; q < 2; q++) { const int i = (l + 64 * q) * 16; if (i < rem) t += rxf[cons0 + nin + i].x; }
                        asm volatile("" :: "v"(t));
                    } else
                    for (int rep = CENSUS_REPS(8); rep > 0; rep--)
                    for (int i = tid; i < RD_RXBUF; i += NT2 - 64) {
                        asm volatile("" ::: "memory");
                        float2 v = sh->rxb[i]; v.x *= rx_sc; v.y *= rx_sc;
                        unsigned hi, lo; rx2_split16(v, hi, lo);
                        sh->rxhl[i] = (u32x2){ hi, lo };
                    }
                }
                if (CENSUS(16)) { int t_ = tm; double f_ = fm; rx2_refine(sh, a.vm, &t_, &f_, t0, tm + 8 - t0, fm - 1.0, fm + 1.0, 0.1, true); __syncthreads(); }
                rx2_refine(sh, a.vm, &tnew, &fhat, t0, tm + 8 - t0, fm - 1.0, fm + 1.0, 0.1, true);
                tm_ref = tnew; fm_ref = dlin2_nc(0.9, fm, 0.1, fhat);                  // radae_rxe.py:206, rounded like the reference's doubles (rade_devutil.h)
                if (tid == 0) { S->tmax = tm_ref; S->fmax = fm_ref; S->lcg = (uint32_t)sh->lcg_next; }
            }
            PH2(9);
            // check_pilots (dsp.py:273-320): 48 pseudo-random rows x {Dt1, Dt2} x 40 frequencies on the f16 matrix cores, one
            // wavefront per (frame, frequency-tile group); then what only depends on refine()'s result: the four correlations at
            // (tmax, fmax) and the frequency-corrected window the demodulator reads
            {
                const int wave = tid >> 6, lane = tid & 63;
                const float rx_unsc = sh->rx_unsc;
                // wavefronts 0 / 1: frame 0 / 1, row tiles 0 and 1; wavefronts 2 / 3: frame 0 / 1, row tile 2, and everything else of the phase -- the four correlations at
                // (tmax, fmax) behind the first table requests, one slice of the frequency-corrected window behind the matrix instructions of every k-step
                const int tm = tm_ref; const double w = 2.0 * PI_D * fm_ref / 8000.0;
                int t2 = tm;
                if (t2 >= RD_NMF - RD_M) t2 -= RD_M;
                if (t2 < RD_M) t2 += RD_M;
                const double rph_th = S->rph_th;
                float2 *cA = sh->cisA[wave & 1], *cB = sh->cisB[wave & 1];
                unsigned *dxh = (unsigned *)sh->xm, *dxl = dxh + 1200;
                const float dx_sc = 0x1p-12f / rx_unsc;           // = the planes' 2^(7 - E): a power of two, the division is exact
                auto pre23 = [=]() {      // (captures by VALUE: by reference the captured locals -- tid among them, reassigned all over the call loop -- stay in scratch memory for the whole kernel: 1700 spills)
                    // rx_phase e^{-jw(n+1)} (complex128 in the reference) = e^{j(theta - w(n+1))} for the 1152 window samples as the product of two small tables --
                    // cisA[a] = e^{j(theta - w(64 a + 1))}, cisB[b] = e^{-j w b}, 82 reduced-angle evaluations per wavefront (each wavefront builds its own copy: no
                    // barrier) -- instead of one evaluation per sample (rounds 2-4: sincosf and the double-precision angle were 1.2 k cycles per 128 samples, more
                    // than half of this phase's wave-cycles)
                    cB[lane] = cis_reduced(-w * (double)lane);
                    if (lane < 18) cA[lane] = cis_reduced(rph_th - w * (double)(64 * lane + 1));
                    // the four correlations at (tmax, fmax): 160 samples over the two wavefronts
                    double cr[8] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
                    for (int rep = CENSUS_REPS(64); rep > 0; rep--)
                    for (int n = tid - 128; n >= 0 && n < RD_M; n += 128) {
                        asm volatile("" ::: "memory");
                        if (rep == 1 && n < 128) { for (int q = 0; q < 8; q++) cr[q] = 0.0; }
                        const float2 cf = cis_reduced(-w * n);
                        const double sn = cf.y, cs = cf.x;
                        const double2 rp = sh->pd[n], re = sh->pendd[n];
                        const int t0s[4] = { tm, tm + RD_NMF, tm + RD_M + RD_NCP, tm + RD_NMF };
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const float2 x = sh->rxb[t0s[q] + n];
                            const double qr = cs * x.x - sn * x.y, qi = -(cs * x.y + sn * x.x);
                            const double2 r = q < 2 ? rp : re;
                            cr[2 * q] += qr * r.x - qi * r.y; cr[2 * q + 1] += qr * r.y + qi * r.x;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 8; q++) cr[q] = wave_sum_f64(cr[q]);
                    if (lane == 0) {
#pragma unroll
                        for (int q = 0; q < 8; q++) sh->corrp[wave][q] = cr[q];
                    }
                };
                // the corrected window goes straight into two binary16 planes (same power-of-two scale as the rx_buf planes): the demodulator DFT reads them as
                // matrix-core operands.  Sample n sits at n + (n >> 5): the six symbols' fragments then start in different banks.  Slice s = samples
                // 128 s + (tid - 128), s = 0..8 (9 x 128 = 1152)
                auto side23 = [=](int sl) {
                    if (sl >= RD_NEOO / 128) return;
                    const int n = 128 * sl + (tid - 128);
                    float2 v = cmul(sh->rxb[t2 - RD_NCP + n], cmul(cA[n >> 6], cB[n & 63]));
                    v.x *= dx_sc; v.y *= dx_sc;
                    rx2_split16(v, dxh[n + (n >> 5)], dxl[n + (n >> 5)]);
                };
                for (int rep = CENSUS_REPS(32); rep > 0; rep--) {
                    asm volatile("" ::: "memory");
                    if (wave < 2) check2_rows_q<2, 5>(sh, a.corrq16, a.corra16, wave, 0, lane, rx_unsc, []() {}, [](int) {});
                    else check2_rows_q<1, 4>(sh, a.corrq16, a.corra16, wave - 2, 2, lane, rx_unsc, pre23, side23);
                }
                PH2(8);
            }
            PH2(11);
            RX2_SYNC();
            PH2(10);
            // From here to the equaliser ONE phase: the fourth wavefront reduces the row sums to the Rayleigh thresholds, decides candidate /
            // end-of-over / slip, runs the state machine and advances the phase accumulator; the other three run the demodulator DFT
            // (none of the decisions feeds it: the corrected window was cut with the slip-adjusted timing above)
            const double w = 2.0 * PI_D * S->fmax / 8000.0;
            if (tid >= NT2 - 64) {
                const int l = tid - (NT2 - 64);
                double r0 = 0.0, r1 = 0.0;
                for (int t = l; t < RD_NMF; t += 64) { r0 += (double)sh->rowsum1[t]; r1 += (double)sh->rowsum2[t]; }
                r0 = wave_sum_f64(r0); r1 = wave_sum_f64(r1);
                if (l == 0) {
                    const int tm = S->tmax;
                    double red[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) red[q] = sh->corrp[2][q] + sh->corrp[3][q];      // (the two wavefronts that cut the correlations: rx2 check phase)
                    const float sr = sigma_r_from_sums(r0, r1);
                    const double D = sqrt(red[0] * red[0] + red[1] * red[1]) + sqrt(red[2] * red[2] + red[3] * red[3]);     // (well inside double's range: no hypot() scaling)
                    const double De = sqrt(red[4] * red[4] + red[5] * red[5]) + sqrt(red[6] * red[6] + red[7] * red[7]);
                    S->Dthresh = (double)(2.0f * sr) * RD_SQRT_NLOG_1EM4_5;
                    const double Dthresh_eoo = (double)(2.0f * sr) * RD_SQRT_NLOG_1EM5_5;
                    S->Dtmax12 = D; S->Dtmax12_eoo = De;
                    const int eoo = De > Dthresh_eoo;
                    S->candidate = D > S->Dthresh; S->endofover = eoo;
                    int nn = RD_NMF, t2 = tm;
                    if (t2 >= RD_NMF - RD_M) { nn = RD_NMF + RD_M; t2 -= RD_M; }
                    if (t2 < RD_M) { nn = RD_NMF - RD_M; t2 += RD_M; }
                    S->nin = nn; S->tmax = t2;
                    S->synced_count++;
                    if (S->synced_count % 8 == 0) { if (S->uw_errors > 7) S->uw_fail = 1; S->uw_errors = 0; S->uw_from_row = S->n_rows; }
                    state_update(0, !eoo, eoo);
                }
                if (l == 1) { const double th = S->rph_th - w * (double)RD_NEOO; S->rph_th = th - 6.283185307179586476925 * rint(th * 0.15915494309189533577); }
            } else {
                // receiver_one (dsp.py:487-526): 160 -> 30 DFT of the six symbols on the f16 matrix cores.  sym[s][c] = sum_n x_s[n] Wfwd[n][c]: with the row
                // R[c] = (wr, -wi interleaved over n) the real part is R . (xr, xi) and the imaginary part R . (xi, -xr), so the A operand is 32 rows (30 carriers, two
                // planes, a.wfwd16 from L2) and the B operand twelve columns: the six symbols' window planes as they are, and with every (re, im) pair turned into
                // (im, -re) in registers (exact).  hi hi + hi lo + lo hi, cross products first (rade_corr2.h's rule): 30 matrix instructions per 16-row tile in three independent chains,
                // one tile each on wavefronts 0 and 1.  (As vector FMAs -- five lanes per carrier, 32 samples each -- this phase was 9 k cycles, and beside a
                // second workgroup the vector ALU is what the two compete for: HISTORY.md 3.9.)
                typedef const __attribute__((address_space(1))) f16x8 glb_f16x8_t;
                const int wave = tid >> 6, lane = tid & 63, col = lane & 15, g = lane >> 4;
                const int sc_ = col < 6 ? col : min(col - 6, 5);
                const unsigned im_var = col >= 6 ? 0xffffffffu : 0u;       // columns 6..11 (and the unused 12..15): the (im, -re) variant
                const unsigned *dxh = (const unsigned *)sh->xm, *dxl = dxh + 1200;
                const float unsc = sh->rx_unsc;
                static_assert(RD_NCP - 16 == 16 && RD_SYM == 192, "padded window index");
                for (int rep = CENSUS_REPS(256); rep > 0; rep--)
                if (wave < 2) {
                    asm volatile("" ::: "memory");
                    const int tile = wave;
                    const unsigned short *pt = a.wfwd16 + ((size_t)tile * 10 * 2 * 64 + lane) * 8;
                    f16x8 Ah[10], Al[10];
#pragma unroll
                    for (int ks = 0; ks < 10; ks++) { Ah[ks] = *(glb_f16x8_t *)(pt + (size_t)(ks * 2) * 512); Al[ks] = *(glb_f16x8_t *)(pt + (size_t)(ks * 2 + 1) * 512); }
                    f32x4 a0 = { 0.0f, 0.0f, 0.0f, 0.0f }, a1 = a0, a2 = a0;
                    u32x4 bh[2], bl[2];
                    auto turn = [&](unsigned v) { const unsigned t = (v >> 16) | (((v & 0xffffu) ^ 0x8000u) << 16); return (t & im_var) | (v & ~im_var); };   // (re, im) -> (im, -re)
                    auto rows = [&](int slot, int ks) {
                        const int idx = 16 + RD_SYM * sc_ + 16 * ks + 4 * g, pp = idx + (idx >> 5);
#pragma unroll
                        for (int j = 0; j < 4; j++) { bh[slot][j] = turn(dxh[pp + j]); bl[slot][j] = turn(dxl[pp + j]); }
                    };
                    rows(0, 0);
#pragma unroll
                    for (int ks = 0; ks < 10; ks++) {
                        if (ks + 1 < 10) rows((ks + 1) & 1, ks + 1);
                        __builtin_amdgcn_sched_barrier(0);
                        a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al[ks], __builtin_bit_cast(f16x8, bh[ks & 1]), a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[ks], __builtin_bit_cast(f16x8, bl[ks & 1]), a1, 0, 0, 0);
                        a2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[ks], __builtin_bit_cast(f16x8, bh[ks & 1]), a2, 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    const f32x4 r = ((a0 + a1) + a2) * unsc;
                    // C layout: column = lane & 15 (symbol, variant), rows 4 g + (0..3) = carriers 16 tile + 4 g + (0..3)
                    if (col < 12) {
                        float *dst = (float *)&sh->sym[sc_][0] + (col >= 6);
#pragma unroll
                        for (int rr = 0; rr < 4; rr++) { const int c = 16 * tile + 4 * g + rr; if (c < RD_NC) dst[2 * c] = r[rr]; }
                    }
                } else if (wave == 2) {
                    // the third wavefront has no part in this phase: it prepares the NEXT call's refine() constants (one double-precision sincos per lane: 4 k cycles
                    // that every wavefront waited for at refine()'s first barrier when they were computed at the top of the call).  fmax is final for this call
                    // (refine() is done, the state machine does not touch it); a call that is not synchronised, or a sync entry, clears the flag.
                    const double fm = S->fmax;
                    refine2_tables_sync(sh, lane, fm - 1.0, fm + 1.0, 0.1);
                    if (lane == 0) S->tab_ok = 1;
                }
            }
            PH2(25);
            RX2_SYNC();
            PH2(12);
            const int endofover = S->endofover, n_rows = n_rows0;
            float *zrow = a.zrows + ((size_t)b * a.dec_rows + n_rows) * RD_LATENT;
            float *eoo_dst = a.eoo_out ? a.eoo_out + (size_t)b * RD_NEOOBITS : nullptr;
            const int call_idx0 = mf0 - 1;
            if (!endofover) {
                if (tid < 2 * RD_NC) {
                    const int i = tid / RD_NC, c = tid - i * RD_NC;
                    const int cm = c == 0 ? 1 : (c == RD_NC - 1 ? RD_NC - 2 : c);
                    const float2 *row = sh->sym[i ? 5 : 0];
                    float2 g0 = make_float2(0.0f, 0.0f), g1 = g0;
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        const float pp = sh->eqP[cm - 1 + k];
                        const float2 h = make_float2(row[cm - 1 + k].x / pp, row[cm - 1 + k].y / pp);
                        g0 = cadd(g0, cmul(sh->eqPmat[c][0][k], h));
                        g1 = cadd(g1, cmul(sh->eqPmat[c][1][k], h));
                    }
                    sh->rp[i][c] = cadd(g0, cmul(g1, sh->eqrot[c]));
                }
                RX2_SYNC();
                if (tid < 128) {
                    const int c = tid & 63;
                    if (tid < 64) {
                        float pm = 0.0f;
                        if (c < RD_NC) {
                            const float2 r0 = sh->rp[0][c], r1 = sh->rp[1][c];
                            const float a0 = hypotf(r0.x, r0.y), a1 = hypotf(r1.x, r1.y); pm = a0 * a0 + a1 * a1;
                        }
                        pm = wave_sum_f32(pm);
                        if (c == 0) {
                            float mag = powf(pm / 60.0f, 0.5f) + 1e-6f;
                            S->mag = (mag * fabsf(sh->eqP[0])) / sh->eq_pg;
                            S->valid_output = 1;
                        }
                    } else {
                        float s1 = 0.0f, s2 = 0.0f;
                        if (c < RD_NC) {
                            const float2 r0 = sh->rp[0][c], pc = sh->sym[0][c];
                            const float2 rc = cmul(pc, unit_conj(r0));
                            const float ap = hypotf(pc.x, pc.y); s1 = ap * ap; s2 = fabsf(rc.y) * fabsf(rc.y);
                        }
                        s1 = wave_sum_f32(s1); s2 = wave_sum_f32(s2);
                        if (c == 0) {
                            const float S1 = s1, S2 = s2 + 1e-12f;
                            float snr = S1 / (2.0f * S2) - 1.0f;
                            if (snr <= 0.0f) snr = 0.1f;
                            float snrdB = 10.0f * log10f(snr);
                            snrdB = (snrdB - 2.513f) / 0.8070f;
                            const float snr3k = snrdB + sh->eq_snrc1 + sh->eq_snrc2;
                            S->snr_est = 0.9f * S->snr_est + 0.1f * snr3k;
                        }
                    }
                }
                RX2_SYNC();
                const float mag = S->mag;
                if (tid < RD_NS * RD_NC) {
                    const int k = 1 + tid / RD_NC, c = tid % RD_NC;
                    const float2 r0 = sh->rp[0][c], r1 = sh->rp[1][c];
                    const float2 slope = make_float2((r1.x - r0.x) / 5.0f, (r1.y - r0.y) / 5.0f);
                    const float2 ch = make_float2(slope.x * (float)k + r0.x, slope.y * (float)k + r0.y);
                    const float2 v = cmul(sh->sym[k][c], unit_conj(ch));
                    const float zr = v.x / mag, zi = v.y / mag;
                    zrow[2 * tid] = zr; zrow[2 * tid + 1] = zi;
                    if (a.trace_z && call_idx0 < a.trace_cap) { float *tz = a.trace_z + ((size_t)b * a.trace_cap + call_idx0) * RD_ZMF; tz[2 * tid] = zr; tz[2 * tid + 1] = zi; }
                }
            } else {
                if (tid < 3 * RD_NC) {
                    const int k = 2 + tid / RD_NC, c = tid % RD_NC;
                    const float pp = tab->P[c], pe = tab->Pend[c];
                    const float2 s = make_float2(sh->sym[0][c].x / pp + sh->sym[1][c].x / pe + sh->sym[5][c].x / pe,
                                                 sh->sym[0][c].y / pp + sh->sym[1][c].y / pe + sh->sym[5][c].y / pe);
                    const float2 v = cmul(sh->sym[k][c], unit_conj(s));
                    if (eoo_dst) { eoo_dst[2 * tid] = v.x; eoo_dst[2 * tid + 1] = v.y; }
                    if (a.trace_z && call_idx0 < a.trace_cap) { float *tz = a.trace_z + ((size_t)b * a.trace_cap + call_idx0) * RD_ZMF; tz[2 * tid] = v.x; tz[2 * tid + 1] = v.y; }
                }
            }
            RX2_SYNC();
        }

        PH2(13);
        // ---- state machine (radae_rxe.py:248-297).  Sync entry needs the whole workgroup for refine().
        const int do_entry = (state == ST_CANDIDATE) && S->entry;
        if (do_entry) {
            const int tm = S->tmax; const double fm = S->fmax;
            const int t0 = max(0, tm - 1);
            int tnew = tm; double fnew = fm;
            for (int i = tid; i < RD_M; i += NT2) sh->pd[i] = make_double2(tab->p[i][0], tab->p[i][1]);    // the FFT area is dead: pilot replica for the direct sums
            rx2_refine(sh, a.vm, &tnew, &fnew, t0, tm + 2 - t0, fm - 10.0, fm + 10.0, 0.25, false);
            if (tid == 0) { S->tmax = tnew; S->fmax = fnew + S->foff_err; S->foff_err = 0.0; }
            RX2_SYNC();
        }
        if (tid == 0 && state != ST_SYNC) state_update(do_entry, S->valid_output, S->endofover);
        if (tid == 0 && a.trace) {
            const int call_idx = S->mf - 2;
            if (call_idx < a.trace_cap) {
                rd_rx_trace *tr = a.trace + (size_t)b * a.trace_cap + call_idx;
                tr->state_before = S->state_before; tr->state_after = S->state; tr->nin_before = S->nin_before; tr->nin_after = S->nin; tr->ret = S->valid_output | (S->endofover << 1);
                tr->tmax = S->tmax; tr->f_ind_max = S->f_ind_max; tr->valid_count = S->valid_count; tr->uw_errors = S->uw_errors; tr->synced_count = S->synced_count;
                tr->snr_int = (int)S->snr_est; tr->fmax = S->fmax; tr->Dthresh = S->Dthresh; tr->Dtmax12 = S->Dtmax12; tr->Dtmax12_eoo = S->Dtmax12_eoo; tr->snrdB_3k_est = S->snr_est;
            }
        }
        if (tid == 0) prepare_next();
        RX2_SYNC();
        PH2(14);
    }

    // ---- write the stream state back
    __syncthreads();
    for (int i = tid; i < RD_RXBUF; i += NT2) { st->rx_buf[i][0] = sh->rxb[i].x; st->rx_buf[i][1] = sh->rxb[i].y; }
    for (int i = tid; i < RD_NMF; i += NT2) { st->rowsum1[i] = sh->rowsum1[i]; st->rowsum2[i] = sh->rowsum2[i]; }
    // band-pass state for the next invocation's pre-pass: on the grid the 102 baseband samples before the consumption point are rebuilt from the
    // input and the block phases (what complex_bpf keeps: dsp.py:96-99); off the grid rx2_bpf_own has kept them in the stream record call by call
    if (S->bpf_grid && S->consumed_inv > 0)
        for (int i = tid; i < 102; i += NT2) { const float2 m = rx2_bpf_mem(a, b, S->nin0, S->consumed_inv - 102 + i); st->bpf.mem[i][0] = m.x; st->bpf.mem[i][1] = m.y; }
    if (tid == 0) {
        st->state = S->state; st->nin = S->nin; st->tmax = S->tmax; st->tmax_candidate = S->tmax_candidate; st->valid_count = S->valid_count;
        st->uw_errors = S->uw_errors; st->synced_count = S->synced_count; st->mf = S->mf; st->f_ind_max = S->f_ind_max;
        st->dec_reset_pending = S->dec_reset_pending; st->has_eoo = S->has_eoo; st->lcg = S->lcg; st->dt_valid = S->dt_valid;
        st->rxmax[0] = S->rxmax_cur; st->rxmax[1] = S->rxmax_h0; st->rxmax[2] = S->rxmax_h1;
        st->fmax = S->fmax; st->foff_err = S->foff_err; st->rx_theta = S->rph_th; { double s_, c_; sincos(S->rph_th, &s_, &c_); st->rx_phase[0] = c_; st->rx_phase[1] = s_; }
        st->Dthresh = S->Dthresh; st->Dtmax12 = S->Dtmax12; st->Dtmax12_eoo = S->Dtmax12_eoo; st->snr_est = S->snr_est;
        if (S->consumed_inv > 0) {
            const float2 ph = S->bpf_grid ? ((const float2 *)a.bpf_chain)[(size_t)b * a.chain_stride + 1 + S->calls_inv] : S->bpf_phase;
            st->bpf.phase[0] = ph.x; st->bpf.phase[1] = ph.y; st->bpf.mem_len = 102; st->bpf.grid_off = S->bpf_grid ? 0 : 1;
        }
        st->consumed += S->consumed_round;
        rnd->n_calls = S->n_calls; rnd->n_rows = S->n_rows; rnd->uw_from_row = S->uw_from_row; rnd->consumed = S->consumed_round;
        rnd->out_base = S->out_base;
        a.acc[b * 4 + 0] = S->consumed_inv; a.acc[b * 4 + 1] = S->calls_inv; a.acc[b * 4 + 2] = S->valid_inv; a.acc[b * 4 + 3] = S->eoo_inv;
        a.status[b * 4 + 0] = S->nin; a.status[b * 4 + 1] = S->state == ST_SYNC; a.status[b * 4 + 2] = (int)S->snr_est; a.status[b * 4 + 3] = S->state;
        if (a.wg_cycles) a.wg_cycles[b] = clock64() - wg_t0;
        if (S->n_calls) atomicAdd(&a.progress[0], S->n_calls);
        if (S->calls_inv < a.max_calls && S->valid_inv < a.feat_cap && S->consumed_inv + S->nin <= avail) atomicAdd(&a.progress[1], 1);
    }
}

// start-of-utterance state of stream blockIdx.x in one launch: the receiver record (radae_rxe.py:128-142), the decoder's / encoder's GRU states and conv
// history rows -- whichever are given.  (Rounds 1-4 issued a kernel + two memsets + two 2-D memsets per reset: five launches of a batch's stream, each of which
// waits for a free slot beside the other batches' receiver workgroups.)
__global__ __launch_bounds__(256) void k_batch_reset(rd_reset_args a)
{
    __builtin_amdgcn_s_setprio(3);
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.st) {
        rd_rx_stream *s = a.st + b;
        float2 *raw = (float2 *)s;
        static_assert(sizeof(rd_rx_stream) % 8 == 0, "rd_rx_stream is cleared in 8-byte pieces");
        for (int i = tid; i < (int)(sizeof(rd_rx_stream) / 8); i += 256) raw[i] = make_float2(0.0f, 0.0f);
    }
    if (a.dec_h) for (int i = tid; i < 5 * 96; i += 256) a.dec_h[((size_t)(i / 96) * a.B + b) * 96 + i % 96] = 0.0f;
    if (a.dec_x) for (int i = tid; i < RD_DEC_W; i += 256) a.dec_x[(size_t)b * a.dec_x_sb + i] = 0.0f;
    if (a.enc_h) for (int i = tid; i < 5 * 64; i += 256) a.enc_h[((size_t)(i / 64) * a.B + b) * 64 + i % 64] = 0.0f;
    if (a.enc_x) for (int i = tid; i < 2 * RD_ENC_W; i += 256) a.enc_x[(size_t)b * a.enc_x_sb + i] = 0.0f;
    if (!a.st) return;
    __syncthreads();
    if (tid == 0) {
        rd_rx_stream *s = a.st + b;
        s->state = ST_SEARCH; s->nin = RD_NMF; s->mf = 1; s->bpf.mem_len = 100; s->lcg = a.seeds ? a.seeds[b] : 1u;
        s->rx_phase[0] = 1.0; s->rx_theta = 0.0; s->bpf.phase[0] = 1.0f; s->foff_err = a.foff_err;
    }
}
extern "C" int rd_launch_reset(const rd_reset_args *a, rd_stream_t s)
{
    if (a->B <= 0) return 0;
    hipLaunchKernelGGL(k_batch_reset, dim3(a->B), dim3(256), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}

// the block phases of an invocation, one thread per stream: P[0] = the phase the stream's last call left, P[k + 1] = P[k] E[len_k - 1] in complex64
// as complex_bpf does from call to call; also resets the stream's off-grid flag (a new invocation starts on the grid)
__global__ __launch_bounds__(64) void k_bpf_chain(rd_bpf_args a)
{
    __builtin_amdgcn_s_setprio(3);                         // a serial chain of ~100 steps on one thread per stream: latency, not throughput
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    if (a.zero_acc) {                                      // the receiver's per-invocation counters (rade_batch_rx)
        ((int4 *)a.zero_acc)[b] = make_int4(0, 0, 0, 0);
        if (b == 0) *(int4 *)a.zero_progress = make_int4(0, 0, 0, 0);
    }
    rd_bpf_state *s = bpf_state_of(a, b);
    float2 *c = (float2 *)a.chain + (size_t)b * a.chain_stride;
    const int nin0 = bpf_len0_of(a, b), av = bpf_avail_of(a, b);
    c[0] = make_float2(__int_as_float(nin0), __int_as_float(s->mem_len));
    s->grid_off = 0;
    float2 P = make_float2(s->phase[0], s->phase[1]);
    // the two step factors in registers: a load inside the loop waits for the store before it as well (one counter, in order), i.e. a full
    // memory round trip per block on a serial chain of ~100
    const float2 e0 = ld2(a.tab->bpf_E, min(max(nin0, 1), RD_NEOO) - 1), e1 = ld2(a.tab->bpf_E, RD_NMF - 1);
    int start = 0;
    for (int k = 0; k + 1 < a.chain_stride; k++) {
        c[1 + k] = P;
        if (start >= av) break;                            // P of the first block beyond the input: the phase after the last whole call
        P = cmul_nc(P, k ? e1 : e0);
        start += k ? RD_NMF : nin0;
    }
}
// after a whole invocation was filtered and consumed (the transmit side: every sample is): the state complex_bpf would hold now (dsp.py:96-99)
__global__ __launch_bounds__(128) void k_bpf_advance(rd_bpf_args a)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    rd_bpf_state *s = bpf_state_of(a, b);
    const float2 *c = (const float2 *)a.chain + (size_t)b * a.chain_stride;
    const int nin0 = __float_as_int(c[0].x), n = bpf_avail_of(a, b);
    if (n < 102 || nin0 <= 0) return;                    // (blocks are whole modem / end-of-over frames)
    const float2 *x = (const float2 *)a.x + (size_t)b * a.x_stride;
    if (tid < 102) { const float2 m = bpf_baseband(x, c, a.tab, nin0, n - 102 + tid); s->mem[tid][0] = m.x; s->mem[tid][1] = m.y; }
    if (tid == 0) { const int nb = n <= nin0 ? 1 : 1 + (n - nin0 + RD_NMF - 1) / RD_NMF; s->phase[0] = c[1 + nb].x; s->phase[1] = c[1 + nb].y; s->mem_len = 102; }
}

// complex_bpf.bpf for BPF_BPW consecutive blocks of stream blockIdx.y: the window [102 earlier baseband samples | the block mixed down] staged as binary16
// planes in LDS, one 256-output tile per wavefront on the matrix cores (bpf_fir_tile), mix up, store.  HBM-bound by design (8 bytes in, 8 out per
// sample), so the loop is built around the memory system: the NEXT block's samples are requested before this block is staged (the round trip hides under
// the staging, the matrix instructions and the stores), the block's last 102 baseband samples are handed to the next block through LDS (they are its
// filter memory: nothing is read twice), and the phase-table entries a thread needs are the same for every block (loaded once).
#define BPF_NT 256
#define BPF_BPW 8
__global__ __launch_bounds__(BPF_NT, 4) void k_bpf_fir(rd_bpf_args a)      // (at most 128 registers: two of its wavefronts fit on a SIMD beside a receiver wavefront)
{
    const rd_tables *tab = a.tab; const unsigned short *tab16 = a.bpf16;
    const float2 *rx = (const float2 *)a.x; const long rx_stride = a.x_stride; float2 *rxf = (float2 *)a.y; const long rxf_stride = a.y_stride;
    const float2 *chain = (const float2 *)a.chain; const int chain_stride = a.chain_stride;
    __shared__ BpfLds pl;
    __shared__ unsigned maxw;
    __shared__ float2 tailbuf[102];
    const int k0 = blockIdx.x * BPF_BPW, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float2 *c = chain + (size_t)b * chain_stride;
    // first round trip: the block grid's header, the first block's phases (their addresses do not depend on the header), the taps, the phase-table entries
    const float2 hdr = c[0];
    float2 Pk = c[1 + k0];
    const float2 Pp = c[k0 ? k0 : 1];
    const int av = bpf_avail_of(a, b);
    BpfTaps taps; bpf_load_taps(taps, tab16, lane);
    const int i0 = 16 * (lane & 15) + 4 * (lane >> 4);    // this lane's four outputs inside a tile
    float2 eb[BPF_NQ], eo[4];
#pragma unroll
    for (int q = 0; q < BPF_NQ; q++) eb[q] = ld2(tab->bpf_E, min(tid + 256 * q, RD_NEOO - 1));
#pragma unroll
    for (int r = 0; r < 4; r++) eo[r] = ld2(tab->bpf_E, 256 * wave + i0 + r);
    const int nin0 = __float_as_int(hdr.x), ml0 = __float_as_int(hdr.y);
    if (nin0 <= 0) return;
    int sk = k0 ? nin0 + (k0 - 1) * RD_NMF : 0;
    if (sk >= av) return;
    const float2 *x = rx + (size_t)b * rx_stride;
    const rd_bpf_state *s = bpf_state_of(a, b);
    // second round trip: the first block's samples in one batch (clamped addresses, values dropped afterwards: no branch around a load), and its filter memory
    int n = min(k0 ? RD_NMF : nin0, av - sk);              // (a partial last block is filtered too; no call will consume it)
    float2 xb[BPF_NQ], head = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int q = 0; q < BPF_NQ; q++) xb[q] = x[sk + min(tid + 256 * q, n - 1)];
    if (tid < 102) {
        if (k0) { const int sp = k0 > 1 ? sk - RD_NMF : 0, q = sk - 102 + tid; head = cmul_nc(x[q], cmul_nc(Pp, ld2(tab->bpf_E, q - sp))); }
        else { const int mi = ml0 - 102 + tid; if (mi >= 0) head = make_float2(s->mem[mi][0], s->mem[mi][1]); }
    }
    for (int kk = 0; kk < BPF_BPW; kk++) {
        const int k = k0 + kk;
        const int o = (k == 0 && ml0 == 100) ? 2 : 0;      // before the first call the memory is two samples shorter (dsp.py:55)
        float2 body[BPF_NQ];
#pragma unroll
        for (int q = 0; q < BPF_NQ; q++) { body[q] = cmul_nc(xb[q], cmul_nc(Pk, eb[q])); if (tid + 256 * q >= n) body[q] = make_float2(0.0f, 0.0f); }
        // the next block's samples and phase: in flight from here on
        const int sk2 = sk + (k ? RD_NMF : nin0);
        const bool more = kk + 1 < BPF_BPW && sk2 < av;    // uniform
        const int n2 = more ? min(RD_NMF, av - sk2) : 1;
        const float2 Pn = c[1 + k + (more ? 1 : 0)];
        if (more) {
#pragma unroll
            for (int q = 0; q < BPF_NQ; q++) xb[q] = x[sk2 + min(tid + 256 * q, n2 - 1)];
        }
        const float unsc = bpf_stage_planes(&pl, &maxw, tid, head, body, o);
        // this block's last 102 baseband samples are the next block's filter memory
#pragma unroll
        for (int q = 0; q < BPF_NQ; q++) { const int ti = tid + 256 * q - (n - 102); if (ti >= 0 && ti < 102) tailbuf[ti] = body[q]; }
        if (n < 102 && tid >= n && tid < 102) tailbuf[tid - n] = head;      // a block shorter than the memory: the rest of it is the end of this block's own memory (uniform; no call of the engine's makes one)
        float2 *dst = rxf + (size_t)b * rxf_stride + sk;
        for (int tile = wave; tile < BPF_TILES(n); tile += BPF_NT / 64) {
            f32x4 re, im;
            bpf_fir_tile(&pl, taps, tile, lane, re, im);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = 256 * tile + i0 + r;
                const float2 e = tile == wave ? eo[r] : ld2(tab->bpf_E, min(i, RD_NEOO - 1));     // (a fifth tile only exists for blocks longer than 1024 samples)
                if (i < n) {
                    float2 y = cmul_nc(make_float2(re[r] * unsc, im[r] * unsc), cconj(cmul_nc(Pk, e)));
                    if (a.clip) {                           // np.clip(abs(tx), 0, 1) * exp(1j * angle(tx)) (radae_txe.py:132): the phase kept, the magnitude limited to 1
                        const float m2 = y.x * y.x + y.y * y.y;
                        if (m2 > 1.0f) { const float inv = 1.0f / sqrtf(m2); y.x *= inv; y.y *= inv; }
                    }
                    dst[i] = y;
                }
            }
        }
        if (!more) break;
        __syncthreads();
        if (tid < 102) head = tailbuf[tid];
        sk = sk2; n = n2; Pk = Pn;
    }
}
// the launches of a filtering pass: block phases, the FIR over every block, and (transmit side) the state the filter is left in
extern "C" int rd_launch_bpf(const rd_bpf_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->n_blocks <= 0) return 0;
    hipLaunchKernelGGL(k_bpf_chain, dim3((a->B + 63) / 64), dim3(64), 0, (hipStream_t)s, *a);
    hipLaunchKernelGGL(k_bpf_fir, dim3((a->n_blocks + BPF_BPW - 1) / BPF_BPW, a->B), dim3(BPF_NT), 0, (hipStream_t)s, *a);
    if (a->advance) hipLaunchKernelGGL(k_bpf_advance, dim3(a->B), dim3(128), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}

extern "C" int rd_launch_rx_sync(const rd_sync_args *a, rd_stream_t s)
{
    if (a->B <= 0) return 0;
    hipLaunchKernelGGL(k_rx_sync2, dim3(a->B), dim3(NT2), a->lds_bytes, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}
// dynamic LDS of the receiver kernel (above the 64 KB default): set once per device by rade_batch_open, before any launch
extern "C" int rd_rx_sync_prepare(void)
{
    const int l = (int)sizeof(RxShared2);
    if (hipFuncSetAttribute((const void *)k_rx_sync2, hipFuncAttributeMaxDynamicSharedMemorySize, l) != hipSuccess) return -1;
    return l;
}
