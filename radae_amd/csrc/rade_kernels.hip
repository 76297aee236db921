// rade_kernels.hip -- gfx950 (MI355X) kernels of the RADE hot path + the C launch shims: ONE translation unit (a kernel in a file of its own can change
// another kernel's instructions: tools/codegen_diff.py), one header per stage.
//
// Kernel inventory (reference op each one replaces):
//  rade_gemm.h
//   k_gemm<NT>      f32 MFMA (v_mfma_f32_32x32x2_f32) skinny-N GEMM with fused bias/tanh/GLU epilogue: every Linear / GRU-input /
//                   Conv1d(k=2) / GLU layer of CoreEncoder / CoreDecoder, for all streams and all time steps of a chunk at once
//                   (radae_base.py:260-286, :400-416; src/rade_enc.c:55-114; src/rade_dec.c:50-102)
//   k_gemm16 / k_gemm16p / k_gemm_splitk   the same GEMM on the f16 matrix cores (two binary16 planes), pipelined, and split over K for few rows
//  rade_gru_scan.h
//   k_gru_scan<H>   the serial part of a GRU layer: h_t = f(gi_t, W_hh h_{t-1}); one workgroup per
//                   stream, W_hh rows held in VGPRs, h in LDS (radae_base.py:97-108)
//  rade_rows.h
//   k_enc_pack      12x36 feature frames -> 3x(4x21) encoder input rows, aux symbol -1 (radae_txe.py:114-121)
//   k_pad_rows / k_carry_rows   zero-padding of GEMM inputs to K % 8 == 0; the conv history rows carried to the next chunk
//  rade_ofdm_mod.h
//   k_ofdm_mod      QPSK map, pilot row, 30->160 IDFT, cyclic prefix, tanh PA limiter (dsp.py:340-378); k_ofdm_mod_mp: with the
//                   two-path multipath model and the power sums of the channel folded in
//   k_eoo_build / k_copy_eoo   end-of-over frame with 180 data bits (radae.py:208-219, :441-455)
//  rade_chan.h
//   k_chan_power / k_chan_gain / k_chan_apply   rate-Fs two-path multipath, power normalisation, freq offset, AWGN,
//                   EOO / noise framing (radae.py:529-589, inference.py:263-284)
//   k_multipath_gen / k_multipath_h   Watterson Doppler-spread samples and the rate-Rs channel matrix (doppler_spread.m, multipath_samples.m)
//   k_chan_symbol   symbol-domain channels of the non-OFDM configurations (radae.py:604-634, bbfm.py:157-197)
//   k_noise_probe   philox4x32 and gauss_pair alone on chosen words, for the tests of the generated noise (no caller in the library)
// The receiver (k_rx_sync2, band-pass pre-pass, k_batch_reset) is rade_rx.hip; the batched encoder rade_enc.hip; single-stream steps rade_core_step.hip.
//
// Written for gfx950 only: 64-lane wavefronts, MFMA f32 32x32x2, LDS-resident per-stream working sets.
#include "rade_devutil.h"

__device__ float g_zero_row[2048];   // tap-0 source of a conv row whose decoder state was just reset

#include "rade_gemm.h"
#include "rade_gru_scan.h"
#include "rade_rows.h"
#include "rade_ofdm_mod.h"
#include "rade_chan.h"
