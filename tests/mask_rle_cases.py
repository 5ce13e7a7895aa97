"""Seeded binary planes the CPU and GPU tests of the run-length encoder share (csrc/mask_rle.hip, models/ops/functions/
mask_rle_func.py), and the logits-form inputs built on tests/mask_tail_ref.py.

CHUNK is the number of pixels of the column-major order one workgroup owns (ocpg_mask_rle_query; the GPU test asserts the two
agree): the chunk-boundary planes are built from it."""
import functools

import numpy as np
import torch

import mask_tail_ref as R

CHUNK = 4096


def _from_flat(flat, h, w):
    """A column-major pixel sequence -> the row-major [h, w] plane."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(flat, dtype=np.uint8).reshape((h, w), order="F")))


def _bernoulli(h, w, seed, p=0.5):
    return (torch.rand(h, w, generator=torch.Generator().manual_seed(seed)) < p).to(torch.uint8)


def _blobs(h, w, seed):
    """A coarse uniform field, nearest-upsampled by 16 and thresholded, with 300 columns cleared: in column order runs that cross
    word and chunk boundaries, one longer than 2^16, and shorter runs after longer ones (negative deltas)."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand((h + 15) // 16 + 1, (w + 15) // 16 + 1, generator=g) > 0.5
    m = coarse.repeat_interleave(16, 0).repeat_interleave(16, 1)[5:5 + h, 3:3 + w].clone()
    m[:, 100:400] = False
    return m.to(torch.uint8)


@functools.lru_cache(maxsize=None)
def planes():
    """name -> uint8 [H, W] plane of 0 / 1 (built once per process; do not modify)."""
    out = {
        "1x1-set": torch.ones(1, 1, dtype=torch.uint8),
        "1x1-clear": torch.zeros(1, 1, dtype=torch.uint8),
        "all-clear": torch.zeros(7, 9, dtype=torch.uint8),               # one run
        "all-set": torch.ones(7, 9, dtype=torch.uint8),                  # [0, N]
        "1x130": _bernoulli(1, 130, 1),
        "130x1": _bernoulli(130, 1, 2),
        "63x5": _bernoulli(63, 5, 3),                                    # the word boundary against the column boundary
        "64x5": _bernoulli(64, 5, 4),
        "65x5": _bernoulli(65, 5, 5),
        "bernoulli-37x53": _bernoulli(37, 53, 6),                        # N = 1961, no multiple of 64; transitions everywhere
        "checker-from-0": _from_flat(np.arange(9 * 11) % 2, 9, 11),      # N runs
        "checker-from-1": _from_flat((np.arange(9 * 11) + 1) % 2, 9, 11),   # N + 1 runs
        "blobs-300x700": _blobs(300, 700, 7),
    }
    # 64 x 200 = 12800 pixels = 3 chunks and a part: runs placed against the chunk starts
    n = 64 * 200
    flat = np.zeros(n, dtype=np.uint8)
    flat[CHUNK:CHUNK + 4] = 1                 # a run that starts exactly on a chunk start
    flat[2 * CHUNK - 300:2 * CHUNK] = 1       # ... and one that ends exactly there
    flat[3 * CHUNK] = 1                       # a single pixel on a chunk start
    out["chunk-start-transitions"] = _from_flat(flat, 64, 200)
    flat = np.zeros(n, dtype=np.uint8)
    flat[CHUNK - 3:CHUNK + 5] = 1             # the chunk-start pixel continues the previous chunk's run (set)
    flat[2 * CHUNK + 1:2 * CHUNK + 70] = 1    # ... (clear), with the first transition one pixel in
    flat[3 * CHUNK - 64:] = 1                 # a whole word before the chunk start, to the end of the plane
    out["chunk-start-continues"] = _from_flat(flat, 64, 200)
    return out


def other_bytes(plane, seed=9):
    """The same mask with its set pixels as arbitrary non-zero bytes."""
    v = torch.randint(1, 256, plane.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(torch.uint8)
    return torch.where(plane != 0, v, torch.zeros_like(v))


# ---- the logits form ----------------------------------------------------------------------------------------------------------------
SEED = 11
THR = 0.5
# the binary cases of tests/mask_tail_ref.py, the saturated case and the every-clamp case, each as the file has it and once more at
# the other replication factor (same source, the crop scaled with the virtual map).  The saturated source at up 1 takes crop width 9,
# not 33 // 4 = 8: with 8 the output columns 17 and 52 sample exactly midway between two source columns, where +100 and -100 blend
# to a logit of 0 -- undecidable by construction, whatever the seed.
_OWN = list(R.BINARY_CASES) + [R.CASES[6], R.CASES[3]]
_OTHER = [(1, (4, 6)), (4, (8, 1200)), (1, (20, 25)), (1, (5, 9)), (1, (1, 1))]
LOGIT_CASES = _OWN + [(c[0], up, crop, c[3], c[4]) for c, (up, crop) in zip(_OWN, _OTHER)]
OPEN_CAP = 5e-3          # the share of a plane the fp64 referee may leave undecided: the cap of that file's label cases


@functools.lru_cache(maxsize=None)
def logit_inputs(index):
    """-> (src [N, hs, ws] fp32, up, crop, out, want bool [N, oh, ow] at THR without invert, decided bool [N, oh, ow])."""
    shape, up, crop, out, kind = LOGIT_CASES[index]
    src = R.logits(shape, kind, SEED)
    want, decided = R.binary_decision(R.referee(src, up, crop, out), THR)
    return src, up, crop, out, want, decided


# ---- the post-processors -------------------------------------------------------------------------------------------------------------
def post_outputs(b=2, q=5, seed=31):
    """-> (model outputs with 20 x 36 mask logits, original sizes, augmented sizes) for B = 2 samples of Q = 5 queries."""
    masks = R.logits((b * q, 20, 36), "smooth", seed).view(b, 1, q, 20, 36)
    scores = torch.randn(b, 1, q, 1, generator=torch.Generator().manual_seed(seed))
    return {"pred_logits": scores, "pred_masks": masks}, torch.tensor([(40, 53), (37, 71)]), torch.tensor([(20, 36), (18, 33)])
