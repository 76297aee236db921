"""radae_amd/csrc/rade_model_geom.h -- the one statement of the encoder's and decoder's layer shapes in the C and HIP sources -- held to the shapes of the independent
float64 model (tests/core_ref.py on the shipped blob, which states the geometry on its own), and to what rd_model_parse returns for the three blobs under weights/.
The header's values come from the host compiler (c_decl.c_values), so the per-layer expressions are evaluated as the sources evaluate them.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import c_decl
import core_ref
import dev_abi
from radae_amd import dnnw

CSRC = os.path.join(dev_abi.REPO, "radae_amd", "csrc")
WEIGHTS = os.path.join(dev_abi.REPO, "weights")
BLOBS = {"model19_check3.bin": 84, "model05.bin": 80, "bbfm_random_seed20240501.bin": 80}      # feature-row width: 4 x 21 with the aux symbol, 4 x 20 without
LAYERS = range(5)
PER_LAYER = ("RM_ENC_GRU_IN", "RM_ENC_CONV_IN", "RM_ENC_DIL", "RM_DEC_GRU_IN", "RM_DEC_CONV_IN")
SCALARS = ("RM_NL", "RM_LATENT", "RM_FEAT_AUX", "RM_FEAT", "RM_NFEAT", "RM_STEP_FRAMES", "RM_FILE_FRAME", "RM_FEAT_PAD", "RM_ENC_D1", "RM_ENC_H", "RM_ENC_G", "RM_ENC_CONV",
           "RM_ENC_W", "RM_DEC_D1", "RM_DEC_H", "RM_DEC_G", "RM_DEC_GLU", "RM_DEC_CONV", "RM_DEC_W", "RD_ENC_W", "RD_DEC_W", "RD_ENC_IN", "RD_LATENT", "RD_FEAT_MF",
           "TR_H", "TR_G", "TR_OUT", "TR_NL", "TR_SAVE")


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    """name -> value, and name -> [value of name(l) for the five layers]"""
    exprs = list(SCALARS) + [f"{m}({l})" for m in PER_LAYER for l in LAYERS]
    v = c_decl.c_values([os.path.join(CSRC, "rade_dev.h"), os.path.join(CSRC, "rade_train.h")], exprs, dev_abi.INCLUDE_DIRS, str(tmp_path_factory.mktemp("geom")))
    return {**{s: v[s] for s in SCALARS}, **{m: [v[f"{m}({l})"] for l in LAYERS] for m in PER_LAYER}}


def test_the_header_has_the_float64_models_shapes(geom):
    g = geom
    m = dnnw.load_model(os.path.join(WEIGHTS, "model19_check3.bin"))
    enc, dec = core_ref.Encoder(m), core_ref.Decoder(m)
    z, x = dec.step(np.zeros(g["RM_LATENT"]))                   # a step of either model runs: every product's shapes agree with the concat row it reads
    assert enc.step(np.zeros(g["RM_FEAT_AUX"])).shape == (g["RM_LATENT"],) and z.shape == (g["RM_FEAT_AUX"],) and x.shape == (g["RM_DEC_W"],)
    assert g["RM_NL"] == len(enc.gru) == len(enc.conv) == len(dec.gru) == len(dec.glu) == len(dec.conv) == len(enc.h) == len(dec.h)
    # the encoder: dense1, per layer the GRU's and the conv's inputs and outputs and the dilation, the concat row, z_dense
    assert enc.d1w.shape == (g["RM_ENC_D1"], g["RM_FEAT_AUX"]) and enc.zw.shape == (g["RM_LATENT"], g["RM_ENC_W"]) and core_ref.ENC_W == g["RM_ENC_W"] == g["RD_ENC_W"]
    assert [u.w_ih.shape for u in enc.gru] == [(g["RM_ENC_G"], k) for k in g["RM_ENC_GRU_IN"]]
    assert all(u.w_hh.shape == (g["RM_ENC_G"], g["RM_ENC_H"]) and h.shape == (g["RM_ENC_H"],) for u, h in zip(enc.gru, enc.h))
    assert [c.w1.shape for c in enc.conv] == [c.w0.shape for c in enc.conv] == [(g["RM_ENC_CONV"], k) for k in g["RM_ENC_CONV_IN"]]
    assert [c.dil for c in enc.conv] == g["RM_ENC_DIL"] == list(dnnw.ENC_DILATION)
    # the decoder: the same, with the GLU between a GRU and the concat row, every conv at dilation 1
    assert dec.d1w.shape == (g["RM_DEC_D1"], g["RM_LATENT"]) and dec.ow.shape == (g["RM_FEAT_AUX"], g["RM_DEC_W"]) and core_ref.DEC_W == g["RM_DEC_W"] == g["RD_DEC_W"]
    assert [u.w_ih.shape for u in dec.gru] == [(g["RM_DEC_G"], k) for k in g["RM_DEC_GRU_IN"]]
    assert all(u.w_hh.shape == (g["RM_DEC_G"], g["RM_DEC_H"]) and h.shape == (g["RM_DEC_H"],) for u, h in zip(dec.gru, dec.h))
    assert all(w.shape == (g["RM_DEC_GLU"], g["RM_DEC_H"]) for w in dec.glu)
    assert [c.w1.shape for c in dec.conv] == [(g["RM_DEC_CONV"], k) for k in g["RM_DEC_CONV_IN"]] and all(c.dil == 1 for c in dec.conv)
    # the feature rows: what reaches features_out of a decoder row, the frame of a feature file, the encoder's padded input row
    assert len(core_ref.VISIBLE) == g["RM_FEAT"] == g["RM_STEP_FRAMES"] * g["RM_NFEAT"] and core_ref.UW_COL == g["RM_NFEAT"] and g["RD_LATENT"] == g["RM_LATENT"]
    assert core_ref.rows_to_features(np.zeros((3, g["RM_FEAT_AUX"]))).shape == (1, 3 * g["RM_STEP_FRAMES"] * g["RM_FILE_FRAME"]) == (1, g["RD_FEAT_MF"])
    assert g["RD_ENC_IN"] == g["RM_FEAT_PAD"] == -(-g["RM_FEAT_AUX"] // 16) * 16
    # the training code's names
    assert (g["TR_H"], g["TR_G"], g["TR_OUT"], g["TR_NL"], g["TR_SAVE"]) == (g["RM_DEC_H"], g["RM_DEC_G"], g["RM_FEAT_AUX"], g["RM_NL"], 5 * g["RM_DEC_H"])


@pytest.mark.parametrize("blob", list(BLOBS))
def test_the_host_reader_accepts_the_shipped_blobs_with_the_headers_shapes(geom, blob):
    g = geom
    lib = dev_abi.load()
    data = open(os.path.join(WEIGHTS, blob), "rb").read()
    m = dev_abi.Model()
    assert lib.rd_model_parse(data, len(data), C.byref(m)) == 0
    try:
        assert [(u.n_in, u.hid) for u in m.enc_gru] == [(k, g["RM_ENC_H"]) for k in g["RM_ENC_GRU_IN"]]
        assert [(u.n_in, u.hid) for u in m.dec_gru] == [(k, g["RM_DEC_H"]) for k in g["RM_DEC_GRU_IN"]]
        assert [(c.n_in, c.n_out) for c in m.enc_conv] == [(2 * k, g["RM_ENC_CONV"]) for k in g["RM_ENC_CONV_IN"]]      # both taps side by side
        assert [(c.n_in, c.n_out) for c in m.dec_conv] == [(2 * k, g["RM_DEC_CONV"]) for k in g["RM_DEC_CONV_IN"]]
        assert all((u.n_in, u.n_out) == (g["RM_DEC_H"], g["RM_DEC_GLU"]) for u in m.dec_glu)
        feat = BLOBS[blob]
        assert feat in (g["RM_FEAT_AUX"], g["RM_FEAT"])
        assert (m.enc_dense1.n_in, m.enc_dense1.n_out, m.enc_zdense.n_in, m.enc_zdense.n_out) == (feat, g["RM_ENC_D1"], g["RM_ENC_W"], g["RM_LATENT"])
        assert (m.dec_dense1.n_in, m.dec_dense1.n_out, m.dec_output.n_in, m.dec_output.n_out) == (g["RM_LATENT"], g["RM_DEC_D1"], g["RM_DEC_W"], feat)
    finally:
        lib.rd_model_free(C.byref(m))
