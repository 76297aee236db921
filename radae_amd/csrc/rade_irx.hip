// rade_irx.hip -- the fixed-timing rate-Fs receiver of RADAE.forward / RADAE.receiver (radae.py:312-420, :590-657): known timing, optional correction of a known
// frequency offset, cyclic prefix removal, the 160 -> 30 DFT, the pilot EQ of do_pilot_eq, the QPSK demapper (the frame body: irx_frame of rade_irx.h).  Two entries:
// the ideal-timing ("genie") call, rade_batch_rx_ideal, every stream with n_mf frames from its row's first sample,
//   k_irx_demod   one workgroup per (modem frame, stream), like k_ofdm_mod
//   k_irx_scale   one workgroup per stream: coarse_mag (radae.py:376-381) and the ber_test bit-error count (radae.py:653-657)
// and the stored-file call past the acquisition, rade_batch_rx_file / rade_batch_ber_align (rx.py:223-276), every stream with its own first sample, frame count and
// frequency,
//   k_file_demod  one workgroup per (modem frame, stream); frames past the stream's own are written as zeros
//   k_file_scale  coarse_mag over the stream's own frames
//   k_file_ber    rx.py:268-276: one workgroup per (shift, stream) counts the sign errors
// All are small next to the streaming receiver (genie receiver row); the DFT stays on the vector ALU.
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"
#include "rade_irx.h"

// coarse_mag of a stream (radae.py:376-381) by a workgroup of 256: sqrt(mean |rx_pilots|^2) * mag_scale from the frames' pilot powers, summed by thread, by
// wavefront and then over the four wavefronts in ascending order
__device__ __forceinline__ float irx_coarse_mag(const double *part, int n_mf, float mag_scale)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double p = 0.0;
    for (int i = tid; i < n_mf; i += 256) p += part[i];
    p = wave_sum_f64(p);
    if ((tid & 63) == 0) red[tid >> 6] = p;
    __syncthreads();
    const double tot = ((red[0] + red[1]) + red[2]) + red[3];
    return sqrtf((float)(tot / ((double)n_mf * RD_NC))) * mag_scale;
}

// torch.sum(-z * z_hat > 0) (radae.py:654, rx.py:271) over a workgroup of 256.  Integer counts: a thread's own (e, of irx_sign_error), the wavefront's by a fixed
// exchange pattern, the four wavefronts in ascending order
__device__ __forceinline__ bool irx_sign_error(float z_ref, float z_hat) { return -z_ref * z_hat > 0.0f; }
template <class T>
__device__ __forceinline__ T irx_error_count(int e)
{
    __shared__ T cnt[4];
    const int tid = threadIdx.x;
    for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off);
    if ((tid & 63) == 0) cnt[tid >> 6] = e;
    __syncthreads();
    return ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
}

// rx * conj(lin_phase), radae.py:594-595: the channel's own float32 phase; a stream with freq_offset 0 is not corrected
struct irx_mix_ideal {
    float f0, dfdt;
    __device__ __forceinline__ float2 operator()(float2 v, int n) const
    {
        if (f0 != 0.0f) { float sn, cs; sincosf((float)chan_phase_acc(n, f0, dfdt), &sn, &cs); v = cmul(v, make_float2(cs, -sn)); }
        return v;
    }
};

__global__ __launch_bounds__(192) void k_irx_demod(rd_irx_args a)
{
    const int mf = blockIdx.x, b = blockIdx.y;
    const irx_mix_ideal mix = { a.foff ? a.foff[b] : 0.0f, a.foff ? a.foff[a.B + b] : 0.0f };
    irx_frame(a.tab, (const float2 *)a.rx + (size_t)b * a.rx_stride, mf, mf == a.n_mf - 1, a.time_offset, a.eq, mix,
              a.z_hat + ((size_t)b * a.n_mf + mf) * RD_ZMF, a.part + (size_t)b * a.n_mf + mf);
}

__global__ __launch_bounds__(256) void k_irx_scale(rd_irx_args a)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool scale = a.coarse_mag && a.eq != RD_IRX_NONE;
    const float mag = scale ? irx_coarse_mag(a.part + (size_t)b * a.n_mf, a.n_mf, a.mag_scale) : 1.0f;
    float *z = a.z_hat + (size_t)b * a.n_mf * RD_ZMF;
    const float *zr = a.z_ref ? a.z_ref + (size_t)b * a.n_mf * RD_ZMF : nullptr;
    int e = 0;
    for (int i = tid; i < a.n_mf * RD_ZMF; i += 256) {
        float v = z[i];
        if (scale) { v = v / mag; z[i] = v; }
        if (zr && irx_sign_error(zr[i], v)) e++;
    }
    if (!a.n_err) return;
    const int tot = irx_error_count<int>(e);
    if (tid == 0) a.n_err[b] = (long long)tot;
}

// rx[start:] * exp(-1j w arange(len)), rx.py:223-228: phase and product in double, rounded once; n counted from the stream's start; w = 0: the stream is not mixed
struct irx_mix_file {
    double w;
    __device__ __forceinline__ float2 operator()(float2 v, int n) const
    {
        if (w != 0.0) {
            double sn, cs; sincos(w * (double)n, &sn, &cs);          // e^{-j w n} = (cs, -sn)
            const double vr = (double)v.x * cs + (double)v.y * sn, vi = (double)v.y * cs - (double)v.x * sn;
            v = make_float2((float)vr, (float)vi);
        }
        return v;
    }
};

__global__ __launch_bounds__(192) void k_file_demod(rd_file_rx_args a)
{
    const int mf = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const rd_file_rx_rec rec = a.rec[b];
    float *zf = a.z_hat + ((size_t)b * a.max_mf + mf) * RD_ZMF;
    double *part = a.part + (size_t)b * a.max_mf + mf;
    if (mf >= rec.n_mf) {                                            // past the stream's own frames: zeros
        if (tid < RD_NS * RD_NC) { zf[2 * tid] = 0.0f; zf[2 * tid + 1] = 0.0f; }
        if (tid == 0) *part = 0.0;
        return;
    }
    const irx_mix_file mix = { rec.w };
    irx_frame(a.tab, (const float2 *)a.x + (size_t)b * a.x_stride + rec.start, mf, mf == rec.n_mf - 1, a.time_offset, a.eq, mix, zf, part);
}

__global__ __launch_bounds__(256) void k_file_scale(rd_file_rx_args a)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n_mf = a.rec[b].n_mf;
    if (n_mf <= 0) return;                                        // uniform
    const float mag = irx_coarse_mag(a.part + (size_t)b * a.max_mf, n_mf, a.mag_scale);
    float *z = a.z_hat + (size_t)b * a.max_mf * RD_ZMF;
    for (int i = tid; i < n_mf * RD_ZMF; i += 256) z[i] = z[i] / mag;
}

// rx.py:268-276 for shift f = blockIdx.x of stream blockIdx.y: the sign errors of z_hat against z_ref[240 f:] over the shorter of the two.  A shift that leaves no
// reference symbol gets -1.
__global__ __launch_bounds__(256) void k_file_ber(rd_file_ber_args a)
{
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const rd_file_ber_rec rec = a.rec[b];
    const long long off = (long long)RD_ZMF * f, left = rec.n_ref - off;
    long long *out = a.n_err + (size_t)b * RD_FILE_NSHIFT + f;
    if (left <= 0) { if (tid == 0) *out = -1; return; }
    const long long n_syms = left < rec.n_hat ? left : rec.n_hat;
    const float *zr = a.z_ref + (size_t)b * a.ref_stride + off, *zh = a.z_hat + (size_t)b * a.hat_stride;
    int e = 0;
    for (long long i = tid; i < n_syms; i += 256) if (irx_sign_error(zr[i], zh[i])) e++;
    const long long tot = irx_error_count<long long>(e);
    if (tid == 0) *out = tot;
}

extern "C" int rd_launch_irx(const rd_irx_args *a, rd_stream_t s)
{
    if (a->B <= 0) return 0;
    if (a->n_mf < 2 || a->time_offset < -RD_NCP || a->time_offset > 0 || a->eq < RD_IRX_LS || a->eq > RD_IRX_NONE || !a->z_hat || !a->part) return -1;
    hipLaunchKernelGGL(k_irx_demod, dim3(a->n_mf, a->B), dim3(192), 0, (hipStream_t)s, *a);
    if ((a->coarse_mag && a->eq != RD_IRX_NONE) || a->z_ref) hipLaunchKernelGGL(k_irx_scale, dim3(a->B), dim3(256), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}

extern "C" int rd_launch_file_rx(const rd_file_rx_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_mf <= 0) return 0;
    if (a->time_offset < -RD_NCP || a->time_offset > 0 || a->eq < RD_IRX_LS || a->eq > RD_IRX_NONE || !a->z_hat || !a->part || !a->rec) return -1;
    hipLaunchKernelGGL(k_file_demod, dim3(a->max_mf, a->B), dim3(192), 0, (hipStream_t)s, *a);
    if (a->coarse_mag && a->eq != RD_IRX_NONE) hipLaunchKernelGGL(k_file_scale, dim3(a->B), dim3(256), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}

extern "C" int rd_launch_file_ber(const rd_file_ber_args *a, rd_stream_t s)
{
    if (a->B <= 0) return 0;
    hipLaunchKernelGGL(k_file_ber, dim3(RD_FILE_NSHIFT, a->B), dim3(256), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}
