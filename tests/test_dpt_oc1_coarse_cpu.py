"""CPU: sizes of the DPT heads' coarse-map output_conv1 (run_dpt's SKIMI_DPT_OC1_COARSE path, vggt_dpt.hip) at the bench's
shape, worked out without a GPU: 32 frames of 518 x 518, refinenet1's map 148 x 148 with 256 features, 128 channels out.
The allocation order is restated from run_dpt; the limits are the ones the launches check (gemm_x3dma_eligible,
dpt_tap_sum_launch) or index with."""
F_, H0, FEAT, IMG = 32, 148, 256, 518
CO = FEAT // 2
M0, M1 = F_ * H0 * H0, F_ * (2 * H0) ** 2


def _a(n):  # the arena's 256-byte granule
    return -(-n // 256) * 256


def test_taps_fit_the_kernels_index_ranges():
    orec = M0 * FEAT * 4                       # out_conv's records, the contraction's A operand
    taps = M0 * 9 * CO * 4                     # [pixel][tap][128] fp32
    assert taps == 3_229_876_224               # 3.23 GB, against 2.87 GB of fine-map records on the other path
    assert M1 * FEAT * 4 == 2_871_001_088
    # gemm_x3dma_eligible: the zero page within a 32-bit lane offset of A, the weight records too
    assert orec + 256 < (1 << 32) - (1 << 28) and 9 * CO * FEAT * 4 < (1 << 32)
    # a chip's worth of 256-row tiles: 2738 row tiles x 4.5 column tiles of 256
    assert M0 >= 4096 and -(-M0 // 256) * -(-9 * CO // 256) >= 160
    # dpt_tap_sum_launch: grid z = frames, 64-bit element offsets in the kernel; the fp32 GEMM epilogue indexes rows x ldo in 64 bits
    assert F_ < 65536 and M0 * 9 * CO < 1 << 62


def test_arena_peak_not_above_the_fine_path():
    """from refinenet1's out_conv to the end of the head (what lies below is the same on both paths): the coarse path holds
    c1 under its records + taps, releases those two, and the tail's 518 x 518 x 32 map takes their place"""
    c1 = _a(M1 * CO * 4)
    tail = _a(F_ * IMG * IMG * 32 * 4)
    fine = _a(M0 * FEAT * 4) + _a(M1 * FEAT * 4 + 256) + c1 + tail          # olow, records (kept to the end), c1, tail
    coarse = c1 + max(_a(M0 * FEAT * 4 + 256) + _a(M0 * 9 * CO * 4), tail)
    assert coarse < fine, (coarse, fine)
