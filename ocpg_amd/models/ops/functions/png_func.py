"""PNG files of 8-bit masks and label maps with a run-length deflate stream: binding of csrc/png_rle.hip (ocpg_png_rle_count /
ocpg_png_rle_emit) and the host composition of the same bytes.

The file: signature, IHDR (8-bit greyscale, or 8-bit palette + PLTE when a palette is given; no interlace), one IDAT, IEND.  The IDAT
data is 78 01, the deflate stream and Adler-32 of the filtered data (filter type 0: every row is 0x00 + its bytes).  The deflate stream
codes every row on its own: a fixed-Huffman block (BFINAL = 0) with the row's tokens and end-of-block, then an empty stored block,
which ends the row on a byte boundary; behind the last row the final block 03 00.  The tokens of a row: its W + 1 filtered bytes cut
into maximal runs of equal bytes; a run of value v and length n is the literal v, (n - 1) // 258 matches of length 258 at distance 1,
then one match of length (n - 1) % 258 at distance 1 when that is >= 3 and that many more literals v otherwise.

GPU tensors run the kernels: the planes never reach the host, only three integers per plane (stream bytes and the two sums Adler-32
is finished from) and the streams do; the host slices, takes one crc32 per file and frames the chunks.  CPU tensors run the vectorised
composition below, so the bytes stay testable without a GPU.  The length of a stream depends on the data, so a call synchronises
twice and cannot be captured.  The files are 2.5 to 6 times the size of Pillow's (about 3.6 times for a smooth blob mask): the
price of rows that can be made in parallel."""
import struct
import zlib

import numpy as np
import torch

from ...._lib import check, lib, stream_ptr

MAX_WIDTH = 4096               # csrc/png_rle.hip: the per-wave bit buffer
_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_LEN_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258])
_LEN_EXTRA = np.array([0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0])


def _reverse(code, nbits):
    """Huffman codes enter the stream most-significant bit first: the value whose bits, taken from the least-significant one, are
    the code's."""
    code = np.asarray(code, dtype=np.int64)
    out = np.zeros_like(code)
    for k in range(16):
        out |= ((code >> k) & 1) << (nbits - 1 - k)              # bits with k >= nbits are clear in every code
    return out


def _literal(v):
    """byte values -> (bits as they enter the stream, count)."""
    v = np.asarray(v, dtype=np.int64)
    nbits = np.where(v < 144, 8, 9)
    return _reverse(np.where(v < 144, 0x30 + v, 0x190 + (v - 144)), nbits), nbits


def _match(length):
    """match lengths 3..258 at distance 1 -> (bits, count): length symbol, extra bits, the five zero bits of distance code 0."""
    length = np.asarray(length, dtype=np.int64)
    i = np.searchsorted(_LEN_BASE, length, side="right") - 1
    sym = 257 + i
    sbits = np.where(sym < 280, 7, 8)
    code = _reverse(np.where(sym < 280, sym - 256, 0xC0 + (sym - 280)), sbits)
    return code | ((length - _LEN_BASE[i]) << sbits), sbits + _LEN_EXTRA[i] + 5


def deflate_rle(plane) -> bytes:
    """uint8 [H, W] -> the deflate stream of its filtered data under the rule above (what the kernels emit)."""
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    h, w = plane.shape
    n = w + 1
    data = np.zeros((h, n), dtype=np.int64)
    data[:, 1:] = plane
    start = np.ones((h, n), dtype=bool)                          # a run never crosses a row: position 0 of every row starts one
    start[:, 1:] = data[:, 1:] != data[:, :-1]
    flat = np.flatnonzero(start.reshape(-1))
    value = data.reshape(-1)[flat]
    length = np.diff(np.append(flat, h * n))
    r = length - 1
    k, rem = r // 258, r % 258
    # pieces (key, bits, count): the key orders them; 8 slots per filtered position, a row's header before and its tail behind its runs
    lit, lit_n = _literal(value)
    keys, vals, cnts = [flat * 8 + 1], [lit], [lit_n]
    full = np.repeat(np.arange(len(flat)), k)
    m258, m258_n = _match(np.full(len(full), 258))
    keys.append(flat[full] * 8 + 2), vals.append(m258), cnts.append(m258_n)
    tail = np.flatnonzero(rem >= 3)
    mt, mt_n = _match(rem[tail])
    keys.append(flat[tail] * 8 + 3), vals.append(mt), cnts.append(mt_n)
    more = np.repeat(np.arange(len(flat)), np.where(rem < 3, rem, 0))
    keys.append(flat[more] * 8 + 3), vals.append(lit[more]), cnts.append(lit_n[more])
    run_bits = lit_n + 13 * k + np.where(rem >= 3, 0, rem * lit_n)
    run_bits[tail] += mt_n
    first = np.searchsorted(flat, np.arange(h) * n)              # every row's first run
    row_bits = 3 + np.add.reduceat(run_bits, first)
    rows = np.arange(h) * n
    keys.append(rows * 8), vals.append(np.full(h, 2)), cnts.append(np.full(h, 3))                        # BFINAL 0, BTYPE 01: bits 0, 1, 0
    pad = (-(row_bits + 10)) % 8                                 # end-of-block (7) + stored header (3), then to the byte boundary
    keys.append((rows + w) * 8 + 6), vals.append(np.zeros(h, dtype=np.int64)), cnts.append(10 + pad)
    keys.append((rows + w) * 8 + 7), vals.append(np.full(h, 0xFFFF0000)), cnts.append(np.full(h, 32))   # 00 00 FF FF
    keys.append(np.array([h * n * 8])), vals.append(np.array([3])), cnts.append(np.array([16]))          # the final block: 03 00
    key, val, cnt = np.concatenate(keys), np.concatenate(vals).astype(np.int64), np.concatenate(cnts).astype(np.int64)
    order = np.argsort(key, kind="stable")
    val, cnt = val[order], cnt[order]
    at = np.cumsum(cnt) - cnt
    total = int(at[-1] + cnt[-1])
    which = np.arange(total) - np.repeat(at, cnt)
    bits = (np.repeat(val, cnt) >> which) & 1
    return np.packbits(bits.astype(np.uint8), bitorder="little").tobytes()


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def _frame(h, w, palette, stream, adler):
    """The file around one deflate stream."""
    head = _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 3 if palette is not None else 0, 0, 0, 0))
    if palette is not None:
        head += _chunk(b"PLTE", bytes(palette))
    return _SIGNATURE + head + _chunk(b"IDAT", b"\x78\x01" + stream + struct.pack(">I", adler)) + _chunk(b"IEND", b"")


def adler_from_sums(n, s0, s1) -> int:
    """Adler-32 of n bytes d_0 .. d_(n-1) from S0 = sum(d_i) and S1 = sum(i * d_i), in Python integers."""
    n, s0, s1 = int(n), int(s0), int(s1)
    return (((n + n * s0 - s1) % 65521) << 16) | ((1 + s0) % 65521)


def _device_streams(planes):
    """[N, H, W] uint8 on the GPU -> (N deflate streams, N Adler-32 values): 3 launches, 2 read-backs."""
    n, h, w = planes.shape
    L = lib()
    with torch.cuda.device(planes.device):
        workspace = torch.empty(24 * n * h, dtype=torch.uint8, device=planes.device)
        totals = torch.empty((n, 3), dtype=torch.int64, device=planes.device)
        check(L.ocpg_png_rle_count(planes.data_ptr(), n, h, w, workspace.data_ptr(), totals.data_ptr(), stream_ptr()), "ocpg_png_rle_count")
        totals_host = totals.cpu()                                                        # readback 1: bytes, S0, S1 per plane
        sizes = totals_host[:, 0].tolist()
        cap = sum(sizes)
        out = torch.empty(cap, dtype=torch.uint8, device=planes.device)
        check(L.ocpg_png_rle_emit(planes.data_ptr(), n, h, w, workspace.data_ptr(), totals_host.data_ptr(), out.data_ptr(), cap,
                                  stream_ptr()), "ocpg_png_rle_emit")
        host = out.cpu().numpy()                                                          # readback 2: the streams
    streams, at = [], 0
    for size in sizes:
        streams.append(host[at:at + size].tobytes())
        at += size
    return streams, [adler_from_sums(h * (w + 1), s0, s1) for _, s0, s1 in totals_host.tolist()]


@torch.no_grad()
def png_encode(planes, palette=None) -> list:
    """uint8 [N, H, W] or [H, W] -> N complete PNG files (bytes).  palette: a flat list of 3 n ints (n <= 256): colour type 3 and a PLTE
    chunk; None: 8-bit greyscale.  GPU tensors run the kernels (contiguous, W <= 4096), CPU tensors the host composition of the
    same bytes."""
    if not torch.is_tensor(planes) or planes.dtype != torch.uint8:
        raise ValueError("png_encode: expected a uint8 tensor")
    if planes.dim() == 2:
        planes = planes[None]
    if planes.dim() != 3 or min(planes.shape) < 1:
        raise ValueError(f"png_encode: expected non-empty planes [N, H, W] or [H, W], got {tuple(planes.shape)}")
    if palette is not None:
        palette = [int(c) for c in palette]
        if len(palette) % 3 or not 3 <= len(palette) <= 768 or min(palette) < 0 or max(palette) > 255:
            raise ValueError("png_encode: a palette is 3 n byte values, 1 <= n <= 256")
    n, h, w = (int(s) for s in planes.shape)
    if planes.is_cuda:
        if not planes.is_contiguous():
            raise ValueError("png_encode: a device tensor has to be contiguous")
        if w > MAX_WIDTH:
            raise ValueError(f"png_encode: rows of more than {MAX_WIDTH} bytes are not served on the device")
        streams, adlers = _device_streams(planes)
    else:
        host = planes.numpy()
        streams = [deflate_rle(p) for p in host]
        filtered = np.zeros((n, h, w + 1), dtype=np.uint8)
        filtered[:, :, 1:] = host
        adlers = [zlib.adler32(f.tobytes()) for f in filtered]
    return [_frame(h, w, palette, s, a) for s, a in zip(streams, adlers)]
