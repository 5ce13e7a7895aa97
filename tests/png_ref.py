"""A deliberately naive restatement of the run-length PNG stream, one bit at a time, and the planes the
encoders are tried on.  It shares nothing with ocpg_amd/models/ops/functions/png_func.py: tables are written out, bits are appended
to a Python list, and the check values come from zlib."""
import struct
import zlib

import numpy as np
import torch

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


class Bits:
    def __init__(self):
        self.bits = []

    def raw(self, value, n):
        """header and extra bits: least-significant bit first"""
        for k in range(n):
            self.bits.append((value >> k) & 1)

    def code(self, value, n):
        """Huffman codes: most-significant bit first"""
        for k in reversed(range(n)):
            self.bits.append((value >> k) & 1)

    def symbol(self, s):
        if s <= 143:
            self.code(0x30 + s, 8)
        elif s <= 255:
            self.code(0x190 + (s - 144), 9)
        elif s <= 279:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + (s - 280), 8)

    def match(self, length):
        """a match of `length` at distance 1"""
        i = max(j for j in range(29) if LENGTH_BASE[j] <= length)
        self.symbol(257 + i)
        self.raw(length - LENGTH_BASE[i], LENGTH_EXTRA[i])
        self.code(0, 5)

    def align(self):
        while len(self.bits) % 8:
            self.bits.append(0)

    def tobytes(self):
        assert len(self.bits) % 8 == 0
        return bytes(sum(b << k for k, b in enumerate(self.bits[i:i + 8])) for i in range(0, len(self.bits), 8))


def filtered(plane):
    """uint8 [H, W] numpy -> the filtered data: every row is 0x00 (filter type 0) + its bytes."""
    return b"".join(b"\x00" + bytes(row.tolist()) for row in plane)


def deflate(plane):
    out = Bits()
    for row in plane:
        data = [0] + row.tolist()
        out.raw(0, 1)                                            # BFINAL = 0
        out.raw(1, 2)                                            # BTYPE = 01
        i = 0
        while i < len(data):
            j = i
            while j < len(data) and data[j] == data[i]:
                j += 1
            v, r = data[i], j - i - 1
            out.symbol(v)
            while r >= 258:
                out.match(258)
                r -= 258
            if r >= 3:
                out.match(r)
            else:
                for _ in range(r):
                    out.symbol(v)
            i = j
        out.symbol(256)
        out.raw(0, 3)                                            # an empty stored block
        out.align()
        for byte in (0x00, 0x00, 0xFF, 0xFF):
            out.raw(byte, 8)
    out.raw(1, 1)                                                # BFINAL = 1
    out.raw(1, 2)
    out.symbol(256)
    out.align()
    return out.tobytes()


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def png(plane, palette=None):
    """uint8 [H, W] numpy -> the file."""
    h, w = plane.shape
    data = filtered(plane)
    idat = b"\x78\x01" + deflate(plane) + struct.pack(">I", zlib.adler32(data) & 0xFFFFFFFF)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">II", w, h) + bytes([8, 3 if palette is not None else 0, 0, 0, 0]))
    if palette is not None:
        out += chunk(b"PLTE", bytes(palette))
    return out + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


def chunks(data):
    """a PNG file -> [(type, data)], every length and CRC checked."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        out.append((kind, body))
        at += 12 + n
    assert at == len(data)
    return out


PALETTE = [0, 0, 0, 128, 0, 0, 0, 128, 0, 128, 128, 0, 0, 0, 128]          # five entries


def _seeded(shape, seed, kind):
    g = torch.Generator().manual_seed(seed)
    if kind == "bytes":
        return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    return (torch.rand(shape, generator=g) < 0.3).to(torch.uint8) * 255


def edge_planes():
    """name -> uint8 [H, W] tensor.  Row lengths are counted with the filter byte: W + 1."""
    p = {}
    p["1x1_zero"] = torch.zeros(1, 1, dtype=torch.uint8)
    p["1x1_255"] = torch.full((1, 1), 255, dtype=torch.uint8)
    p["1x5_ramp"] = torch.tensor([[0, 0, 7, 7, 7]], dtype=torch.uint8)
    p["5x1_column"] = torch.tensor([[0], [255], [255], [0], [144]], dtype=torch.uint8)
    p["7x1_zero"] = torch.zeros(7, 1, dtype=torch.uint8)
    for n in (2, 3, 4, 257, 258, 259, 260, 516, 517, 519):               # either side of the 3-byte match and of 258, filter byte included
        p[f"row{n}_zero"] = torch.zeros(2, n - 1, dtype=torch.uint8)      # first byte 0: one run with the filter byte
        p[f"row{n}_255"] = torch.full((2, n - 1), 255, dtype=torch.uint8)     # first byte not 0: the filter byte is a run of its own
    for v in (0, 143, 144, 255):                                         # either side of the 8 / 9-bit literals
        q = torch.full((3, 70), v, dtype=torch.uint8)
        q[1, 5:8] = 143 if v != 143 else 144                             # a run of 3 (two literals), of 62 behind it and of 5 before it
        q[2, 66] = 1
        p[f"value{v}"] = q
    p["every_byte"] = torch.arange(256, dtype=torch.uint8).repeat(2, 2)  # [2, 512]: all literals
    p["alternating"] = torch.tensor([0, 255], dtype=torch.uint8).repeat(3, 100)
    p["alternating_from_255"] = torch.tensor([255, 0, 144], dtype=torch.uint8).repeat(2, 43)
    q = _seeded((4, 131), 1, "bytes")
    q[2] = q[1]                                                          # a row that equals the previous one
    p["repeated_row"] = q
    p["all_255"] = torch.full((5, 300), 255, dtype=torch.uint8)
    p["random_binary_3x259"] = _seeded((3, 259), 2, "binary")
    p["random_binary_4x1300"] = _seeded((4, 1300), 3, "binary")
    p["random_bytes_3x65"] = _seeded((3, 65), 4, "bytes")
    p["runs_over_groups"] = torch.zeros(3, 200, dtype=torch.uint8)        # runs that end at and around positions 63, 64, 127, 128
    p["runs_over_groups"][0, 62:] = 9
    p["runs_over_groups"][1, 63:127] = 200
    p["runs_over_groups"][2, 126] = 1
    p["runs_over_groups"][2, 127] = 2
    p["long_run_2x1100"] = torch.full((2, 1100), 17, dtype=torch.uint8)   # four matches of 258 and a tail
    p["long_run_2x1100"][1, 1034:] = 0                                   # 1 + 1034 = 4 * 258 + 3: r = 1033, tail of 1 (a literal)
    return p


def batch_planes():
    """N = 3 planes of one size with different content."""
    return torch.stack([_seeded((6, 261), 5, "binary"), _seeded((6, 261), 6, "bytes"), torch.zeros(6, 261, dtype=torch.uint8)])


def label_plane():
    """a label map of the objects 0..3 for the palette case."""
    q = torch.zeros(9, 77, dtype=torch.uint8)
    q[1:4, 3:30] = 1
    q[2:8, 20:60] = 2
    q[6:9, 50:77] = 3
    return q
