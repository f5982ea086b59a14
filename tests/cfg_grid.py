"""The cfg values beside the shipped ones that the suite holds to the oracle (tests/test_gpu_cfg_values.py on the device,
tests/test_arch_config.py on the host): `num_filters`, `num_res_blocks`, `exp_rate`, `decay_rate` of the `[Net]` section.

A row is (numFilters, numResBlocks, expRate, decayRate, D) with D = int(numFilters * decayRate), the channels behind the decay convolution
(models/modelsTF.py:182) -- written out so that a reader sees the channel count and a test can assert the host's arithmetic gives it."""

# (F, R, E, decay, D), why it is here
GRID = [
    ((32, 12, 8, 0.5, 16), "measured by tools/cfg_cliff.py; the fused pointwise pair with D != 25; 16-channel 3x3x3 layers"),
    ((32, 12, 8, 0.9, 28), "measured by tools/cfg_cliff.py; D > 26: the pair is un-fused at the shipped F and E"),
    ((32, 3, 8, 0.82, 26), "the largest D the fused kernels accept"),
    ((32, 2, 8, 0.05, 1), "the smallest D"),
    ((32, 5, 4, 0.8, 25), "E = 128: un-fused around the shipped D"),
    ((16, 2, 8, 0.8, 12), "16 -> 16 reducers, mainConv1 1 -> 16, upscaleConv1 16 -> 9"),
    ((64, 1, 8, 0.8, 51), "Cout > 32 everywhere; one block: the backward's flush cadence never fires"),
    ((48, 2, 6, 0.9, 43), "channel counts that are no kernel's instance"),
    ((20, 1, 3, 0.5, 10), "nothing is a multiple of 16"),
    ((32, 0, 8, 0.8, 25), "no residual block at all"),
    ((32, 13, 8, 0.8, 25), "more blocks than shipped on the one-wave-per-SIMD kernels: slot, gblk and slab-region counts"),
]

# the same rows at other frame counts, input channels and batches: (row, numImgLR, isGrayScale, batch)
VARIANTS = [
    ((32, 12, 8, 0.5, 16), 13, True, 2),        # a D = 16 configuration on the five-reducer network
    ((16, 2, 8, 0.8, 12), 7, True, 2),
    ((32, 5, 4, 0.8, 25), 9, False, 2),         # an un-fused configuration on three input channels
    ((32, 3, 8, 0.82, 26), 9, True, 5),         # more per-sample scale slots than two, another strip partition
]


def pw_fused(F, E, D):
    """mfma_pw_supported (csrc/kernels_mfma.hip): the shapes the fused expConv + ReLU + decConv kernels take in families 1 ... 4."""
    return F == 32 and F * E == 256 and 1 <= D <= 26


def arch_of(row, T=9, gray=True):
    F, R, E, decay, _ = row
    return dict(numFilters=F, numResBlocks=R, expRate=E, decayRate=decay, numImgLR=T, inChannels=1 if gray else 3)


def case_id(row, T=9, gray=True, B=2):
    F, R, E, decay, D = row
    s = "f%d-r%d-e%d-d%d" % (F, R, E, D)
    return s + ("" if T == 9 else "-t%d" % T) + ("" if gray else "-rgb") + ("" if B == 2 else "-b%d" % B)
