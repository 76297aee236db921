/*
 * rade_model_geom.h -- the geometry of the radae core encoder and decoder (radae_base.py:223-286, :358-430), stated once.  Plain C, constants and asserts only:
 * included by the host files (.c) and the kernels (.hip) alike, through rade_dev.h.
 *
 * Both networks are a DenseNet-style stack: dense1, then RM_NL layers of (GRU, conv), every layer reading the whole concat row written so far and appending its own
 * columns to it.  The decoder puts a GLU between a GRU and the concat row.  So the GRU of layer l reads d1 + l (H + conv) columns, its conv H more, and the concat
 * row is that expression at l = RM_NL: 864 = 64 + 5 (64 + 96) for the encoder, 736 = 96 + 5 (96 + 32) for the decoder.
 */
#ifndef RADE_MODEL_GEOM_H
#define RADE_MODEL_GEOM_H
#ifndef __cplusplus
#include <assert.h>                   /* static_assert in C11 */
#endif

#define RM_NL          5              /* (GRU, conv) layers of either network */
#define RM_LATENT      80             /* z of one 40 ms step */
/* a step's feature row: four frames of 20 features, with the aux (unique-word) symbol behind each (model19) or without (model05, bbfm) */
#define RM_STEP_FRAMES 4
#define RM_NFEAT       20             /* the features of a frame the networks see */
#define RM_FEAT_AUX    (RM_STEP_FRAMES * (RM_NFEAT + 1))     /* 84 */
#define RM_FEAT        (RM_STEP_FRAMES * RM_NFEAT)           /* 80 */
#define RM_FILE_FRAME  36             /* floats per frame of a feature file; the first RM_NFEAT are used */
#define RM_FEAT_PAD    ((RM_FEAT_AUX + 15) / 16 * 16)        /* the encoder's input row: a whole number of 16-column k-blocks of the f16 matrix instructions */

/* encoder: dense1 | 5 x (GRU 64, conv 96, dilation 1,2,2,2,2) | z_dense */
#define RM_ENC_D1      64             /* dense1 outputs */
#define RM_ENC_H       64             /* GRU hidden units */
#define RM_ENC_G       (3 * RM_ENC_H) /* gate rows, torch's order r, z, n */
#define RM_ENC_CONV    96             /* conv outputs */
#define RM_ENC_DIL(l)  ((l) == 0 ? 1 : 2)
#define RM_ENC_GRU_IN(l)  (RM_ENC_D1 + (l) * (RM_ENC_H + RM_ENC_CONV))     /* columns the GRU of layer l reads */
#define RM_ENC_CONV_IN(l) (RM_ENC_GRU_IN(l) + RM_ENC_H)                    /* and its conv, per tap */
#define RM_ENC_W       RM_ENC_GRU_IN(RM_NL)

/* decoder: dense1 | 5 x (GRU 96, GLU 96, conv 32, dilation 1) | output */
#define RM_DEC_D1      96
#define RM_DEC_H       96
#define RM_DEC_G       (3 * RM_DEC_H)
#define RM_DEC_GLU     RM_DEC_H       /* x sigmoid(W x): as wide as the GRU whose state it gates */
#define RM_DEC_CONV    32
#define RM_DEC_GRU_IN(l)  (RM_DEC_D1 + (l) * (RM_DEC_GLU + RM_DEC_CONV))
#define RM_DEC_CONV_IN(l) (RM_DEC_GRU_IN(l) + RM_DEC_GLU)
#define RM_DEC_W       RM_DEC_GRU_IN(RM_NL)

static_assert(RM_ENC_W == 864 && RM_ENC_W == RM_ENC_D1 + RM_NL * (RM_ENC_H + RM_ENC_CONV), "encoder concat row = dense1 + the five layers' columns");
static_assert(RM_DEC_W == 736 && RM_DEC_W == RM_DEC_D1 + RM_NL * (RM_DEC_GLU + RM_DEC_CONV), "decoder concat row = dense1 + the five layers' columns");
static_assert(RM_ENC_GRU_IN(4) == 704 && RM_DEC_GRU_IN(4) == 608, "GRU input widths 64, 224, 384, 544, 704 and 96, 224, 352, 480, 608");
static_assert(RM_ENC_G == 3 * RM_ENC_H && RM_ENC_G == 192 && RM_DEC_G == 3 * RM_DEC_H && RM_DEC_G == 288, "three gates per hidden unit");
static_assert(RM_FEAT_AUX == 84 && RM_FEAT == 80 && RM_FEAT_PAD == 96 && RM_NFEAT < RM_FILE_FRAME, "feature rows: 4 x 21, 4 x 20, and 84 padded to 16");
static_assert(RM_ENC_CONV_IN(0) % 32 == 0 && RM_DEC_CONV_IN(0) % 32 == 0 && (RM_ENC_H + RM_ENC_CONV) % 32 == 0 && (RM_DEC_GLU + RM_DEC_CONV) % 32 == 0,
              "every GRU and conv input is a whole number of 32-column k-steps of the f16 matrix instructions");
#endif
