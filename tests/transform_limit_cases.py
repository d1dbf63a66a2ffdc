"""Transform limit cases: the shapes of vxrt_transform_stamp that reach 64-bit addressing.  Shared by
tests/test_transform_host.py, which holds every case to the cap it must exceed, and tests/test_gpu_transform.py, which runs
LIMIT_DIMS on the device.

A row of one voxel still takes a 32-bit word, so a stamp one voxel wide has as many words as voxels: LIMIT_DIMS has
2^30 + 2^15 voxels in as many words, more than 2^32 bytes, within VXRT_TRANSFORM_MAX_WORDS = 2^31 words.  Word indices fit 32
bits there and byte offsets do not.  The orientations keep the destination within the cap as well and reach both kernels:
rows moved whole (a destination as large as the source) and both transposed axes (the 2^15 + 1 or 2^15 one-voxel rows of a
slice become one row of as many voxels).  OVER_CAP_DIMS is the first skinny shape refused: 2^31 + 2^16 words in as many
voxels, far below vxrt_region_words' 2^36 voxels."""

LIMIT_DIMS = (1, 1 << 15, (1 << 15) + 1)
LIMIT_ORIENTATIONS = [((0, 2, 1), 0b110), ((1, 0, 2), 0b001), ((2, 1, 0), 0b100)]
OVER_CAP_DIMS = (1, 1 << 16, (1 << 15) + 1)


def pattern_bit(index):
    """the structured pattern: bit 0 of source word `index` (a Python int), the same arithmetic as pattern_words"""
    h = (index * 0x9E3779B1) & 0xFFFFFFFF
    return ((h >> 13) ^ (h >> 22) ^ (index >> 7)) & 1


def pattern_words(torch, n, device="cuda"):
    """n source words on the device: bit 0 the pattern, the 31 padding bits of every one-voxel row set"""
    i = torch.arange(n, dtype=torch.int32, device=device)
    h = i * -1640531535  # 0x9E3779B1 as int32: the product wraps like uint32
    bit = ((h >> 13) ^ (h >> 22) ^ (i >> 7)) & 1  # (arithmetic shifts: the sign bits they copy in lie above bit 0)
    del i, h
    return bit | -2
