"""Synthetic Vorbis stream generator for parity tests (test infrastructure).

The shipped TestFiles only exercise Floor1 + Residue1/2 with 1-2 channels and 256/2048 blocks.  This module
writes *setup headers* for arbitrary configurations (Floor0, Residue0, >2 channels, several coupling steps,
several submaps, block sizes 64..8192, codebooks whose dimension does not divide the partition size, ...)
and fills the audio packets with random bits.  Every codebook is a complete fixed-length prefix code (entries
a power of two), so any bit string decodes to *some* side information: no Huffman encoder is needed, and the
oracle and the product are compared on whatever the bits mean.  (The longcode_* configurations are the exception: their
books are VarBooks with long, sparse, ordered and under-subscribed code lists, and their streams are written by the structured
encoder of tests/vorbis_encode.py, which chooses entries and so writes the long codes.)  Header layouts follow what the reference
parses (StreamDecoder.cs:179-289, Codebook.cs:59-283, Floor0.cs:28-65, Floor1.cs:30-133, Residue0.cs:35-117,
Mapping.cs:16-93, Mode.cs:24-67).
"""
import math

import numpy as np


class BitWriter:
    """LSB-first bit packer (the inverse of DataPacket.ReadBits, DataPacket.cs:150-283)."""

    def __init__(self):
        self.acc = 0
        self.nbits = 0
        self.out = bytearray()

    def write(self, value, bits):
        if bits == 0:
            return
        assert 0 <= value < (1 << bits), (value, bits)
        self.acc |= value << self.nbits
        self.nbits += bits
        while self.nbits >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.nbits -= 8

    def bytes(self):
        out = bytearray(self.out)
        if self.nbits:
            out.append(self.acc & 0xFF)
        return bytes(out)


def ilog(x):
    n = 0
    while x > 0:
        n += 1
        x >>= 1
    return n


def vorbis_float(mantissa, exponent):
    """Pack mantissa * 2**exponent the way Utils.ConvertFromVorbisFloat32 unpacks it (Utils.cs:45-59)."""
    sign = 0
    if mantissa < 0:
        sign = 1
        mantissa = -mantissa
    assert mantissa < (1 << 21)
    e = exponent + 788
    assert 0 <= e < 1024
    return (sign << 31) | (e << 21) | mantissa


class Book:
    """Fixed-length complete codebook: `bits` code bits, 2**bits entries."""

    def __init__(self, bits, dims=1, lookup=0, min_me=(0, 0), delta_me=(1, 0), value_bits=4, sequence_p=0, mults=None):
        self.bits, self.dims, self.lookup = bits, dims, lookup
        self.entries = 1 << bits
        self.min_me, self.delta_me, self.value_bits, self.sequence_p, self.mults = min_me, delta_me, value_bits, sequence_p, mults

    def lookup1_values(self):
        r = int(math.floor(math.exp(math.log(self.entries) / self.dims)))
        if math.floor((r + 1) ** self.dims) <= self.entries:
            r += 1
        return r

    def write(self, w, rng):
        w.write(0x564342, 24)
        w.write(self.dims, 16)
        w.write(self.entries, 24)
        w.write(0, 1)  # not ordered
        w.write(0, 1)  # not sparse
        for _ in range(self.entries):
            w.write(self.bits - 1, 5)
        self._write_lookup(w, rng)

    def _write_lookup(self, w, rng):
        w.write(self.lookup, 4)
        if self.lookup == 0:
            return
        w.write(vorbis_float(*self.min_me), 32)
        w.write(vorbis_float(*self.delta_me), 32)
        w.write(self.value_bits - 1, 4)
        w.write(self.sequence_p, 1)
        count = self.lookup1_values() if self.lookup == 1 else self.entries * self.dims
        mults = self.mults if self.mults is not None else rng.integers(0, 1 << self.value_bits, count).tolist()
        assert len(mults) == count, (len(mults), count)
        for m in mults:
            w.write(int(m), self.value_bits)


class VarBook(Book):
    """Codebook with an arbitrary list of codeword lengths (0: the entry is unused), written in one of the three forms a setup
    header can carry (Codebook.cs:76-104): "dense" (five bits per entry, no entry unused), "sparse" (a used flag per entry) or
    "ordered" (runs of equal lengths, rising by one: the list must not fall and has no unused entry).  The lookup part is
    Book's.  Codewords follow from the lengths (spec 3.2.1), so a list may leave the tree under-subscribed."""

    def __init__(self, lengths, encoding="dense", dims=1, lookup=0, min_me=(0, 0), delta_me=(1, 0), value_bits=4, sequence_p=0, mults=None):
        self.lengths = [int(x) for x in lengths]
        assert encoding in ("dense", "sparse", "ordered") and all(0 <= x <= 32 for x in self.lengths) and max(self.lengths) > 0
        if encoding != "sparse":
            assert min(self.lengths) > 0
        if encoding == "ordered":
            assert all(a <= b for a, b in zip(self.lengths, self.lengths[1:]))
        self.encoding = encoding
        self.bits, self.dims, self.lookup = max(self.lengths), dims, lookup
        self.entries = len(self.lengths)
        self.min_me, self.delta_me, self.value_bits, self.sequence_p, self.mults = min_me, delta_me, value_bits, sequence_p, mults

    def write(self, w, rng):
        w.write(0x564342, 24)
        w.write(self.dims, 16)
        w.write(self.entries, 24)
        if self.encoding == "ordered":
            w.write(1, 1)
            cur, i = self.lengths[0], 0
            w.write(cur - 1, 5)
            while i < self.entries:
                cnt = 0
                while i + cnt < self.entries and self.lengths[i + cnt] == cur:
                    cnt += 1
                w.write(cnt, ilog(self.entries - i))
                i += cnt
                cur += 1
        else:
            w.write(0, 1)
            sparse = self.encoding == "sparse"
            w.write(1 if sparse else 0, 1)
            for n in self.lengths:
                if sparse:
                    w.write(1 if n else 0, 1)
                if n:
                    w.write(n - 1, 5)
        self._write_lookup(w, rng)


class IncompleteBook(Book):
    """Like Book, but written sparse with its last entry unused: the all-ones code is unassigned, and a packet that
    contains it makes the reference fault (no overflow list to consult, Codebook.cs:306 -> NullReferenceException)."""

    def write(self, w, rng):
        w.write(0x564342, 24)
        w.write(self.dims, 16)
        w.write(self.entries, 24)
        w.write(0, 1)  # not ordered
        w.write(1, 1)  # sparse
        for i in range(self.entries):
            used = i != self.entries - 1
            w.write(1 if used else 0, 1)
            if used:
                w.write(self.bits - 1, 5)
        w.write(self.lookup, 4)
        if self.lookup == 0:
            return
        w.write(vorbis_float(*self.min_me), 32)
        w.write(vorbis_float(*self.delta_me), 32)
        w.write(self.value_bits - 1, 4)
        w.write(self.sequence_p, 1)
        count = self.lookup1_values() if self.lookup == 1 else self.entries * self.dims
        mults = self.mults if self.mults is not None else rng.integers(0, 1 << self.value_bits, count).tolist()
        for m in mults:
            w.write(int(m), self.value_bits)


def write_floor1(w, partition_classes, class_dims, class_subclass_bits, masterbooks, subclass_books, multiplier, rangebits, xs):
    """Floor1.Init layout (Floor1.cs:30-92).  xs: the X values after the two implicit ones."""
    w.write(1, 16)
    w.write(len(partition_classes), 5)
    for c in partition_classes:
        w.write(c, 4)
    for c in range(max(partition_classes) + 1):
        w.write(class_dims[c] - 1, 3)
        w.write(class_subclass_bits[c], 2)
        if class_subclass_bits[c] > 0:
            w.write(masterbooks[c], 8)
        for j in range(1 << class_subclass_bits[c]):
            w.write(subclass_books[c][j] + 1, 8)  # -1 => unused
    w.write(multiplier - 1, 2)
    w.write(rangebits, 4)
    for x in xs:
        w.write(x, rangebits)


def write_floor0(w, order, rate, bark_map_size, amp_bits, amp_ofs, books):
    """Floor0.Init layout (Floor0.cs:28-49)."""
    w.write(0, 16)
    w.write(order, 8)
    w.write(rate, 16)
    w.write(bark_map_size, 16)
    w.write(amp_bits, 6)
    w.write(amp_ofs, 8)
    w.write(len(books) - 1, 4)
    for b in books:
        w.write(b, 8)


def write_residue(w, rtype, begin, end, psize, classbook, cascades, books):
    """Residue0.Init layout (Residue0.cs:35-66).  books: flat list in (class, stage) order of set cascade bits."""
    w.write(rtype, 16)
    w.write(begin, 24)
    w.write(end, 24)
    w.write(psize - 1, 24)
    w.write(len(cascades) - 1, 6)
    w.write(classbook, 8)
    for c in cascades:
        w.write(c & 7, 3)
        if c >> 3:
            w.write(1, 1)
            w.write(c >> 3, 5)
        else:
            w.write(0, 1)
    for b in books:
        w.write(b, 8)


def write_mapping(w, channels, submaps, coupling, mux, submap_floor_residue):
    """Mapping.Init layout (Mapping.cs:16-78)."""
    w.write(0, 16)
    if submaps > 1:
        w.write(1, 1)
        w.write(submaps - 1, 4)
    else:
        w.write(0, 1)
    if coupling:
        w.write(1, 1)
        w.write(len(coupling) - 1, 8)
        bits = ilog(channels - 1)
        for mag, ang in coupling:
            w.write(mag, bits)
            w.write(ang, bits)
    else:
        w.write(0, 1)
    w.write(0, 2)
    if submaps > 1:
        for c in range(channels):
            w.write(mux[c], 4)
    for fl, rs in submap_floor_residue:
        w.write(0, 8)
        w.write(fl, 8)
        w.write(rs, 8)


def id_header(channels, rate, block0, block1):
    w = BitWriter()
    for b in b"\x01vorbis":
        w.write(b, 8)
    w.write(0, 32)
    w.write(channels, 8)
    w.write(rate, 32)
    w.write(0, 32)
    w.write(0, 32)
    w.write(0, 32)
    w.write(ilog(block0) - 1, 4)
    w.write(ilog(block1) - 1, 4)
    w.write(1, 1)
    return w.bytes()


def comment_header():
    w = BitWriter()
    for b in b"\x03vorbis":
        w.write(b, 8)
    w.write(0, 32)
    w.write(0, 32)
    w.write(1, 1)
    return w.bytes()


def make_stream(cfg, npackets, seed, consistent_windows=True, min_len=16, max_len=220):
    """cfg: dict, see CONFIGS.  Returns (packets, granules, flags): 3 headers + npackets random audio packets."""
    rng = np.random.default_rng(seed)
    ch, b0, b1 = cfg["channels"], cfg["block0"], cfg["block1"]
    w = BitWriter()
    for b in b"\x05vorbis":
        w.write(b, 8)
    books = cfg["books"]
    w.write(len(books) - 1, 8)
    for bk in books:
        bk.write(w, rng)
    w.write(0, 6)   # time count - 1
    w.write(0, 16)
    w.write(len(cfg["floors"]) - 1, 6)
    for f in cfg["floors"]:
        f(w)
    w.write(len(cfg["residues"]) - 1, 6)
    for r in cfg["residues"]:
        r(w)
    w.write(len(cfg["mappings"]) - 1, 6)
    for m in cfg["mappings"]:
        m(w)
    modes = cfg["modes"]  # list of (blockflag, mapping)
    w.write(len(modes) - 1, 6)
    for flag, mp in modes:
        w.write(flag, 1)
        w.write(0, 16)
        w.write(0, 16)
        w.write(mp, 8)
    w.write(1, 1)
    packets = [id_header(ch, cfg.get("rate", 44100), b0, b1), comment_header(), w.bytes()]
    mode_bits = ilog(len(modes) - 1)
    prev_long = None
    seq = rng.integers(0, len(modes), npackets)
    for k in range(npackets):
        pw = BitWriter()
        pw.write(0, 1)
        m = int(seq[k])
        pw.write(m, mode_bits)
        is_long = modes[m][0] == 1
        if is_long:
            if consistent_windows:
                nxt_long = modes[int(seq[k + 1])][0] == 1 if k + 1 < npackets else True
                pf = 1 if (prev_long is None or prev_long) else 0
                pw.write(pf, 1)
                pw.write(1 if nxt_long else 0, 1)
            else:
                pw.write(int(rng.integers(0, 2)), 1)
                pw.write(int(rng.integers(0, 2)), 1)
        prev_long = is_long
        body = rng.integers(0, 256, int(rng.integers(min_len, max_len))).astype(np.uint8)
        # bias: floor "has energy" bits etc. are just random; sprinkle zeros so that some channels stay silent
        if rng.random() < 0.15:
            body[: int(rng.integers(1, 4))] = 0
        for byte in body.tolist():
            pw.write(byte, 8)
        packets.append(pw.bytes())
    return packets, [-1] * len(packets), [0] * len(packets)


# ---- configurations --------------------------------------------------------------------------------

def _floor1_small(class_book, sub_book):
    # 2 partitions of class 0 (dim 2, 1 subclass bit): 6 posts in total
    return lambda w: write_floor1(w, [0, 0], {0: 2}, {0: 1}, {0: class_book}, {0: [sub_book, sub_book]}, 1, 7, [32, 96, 16, 64])


def _floor1_long(class_book, sub_book, rangebits, n_parts=5):
    xs = []
    step = (1 << rangebits) // (2 * n_parts * 2 + 1)
    for i in range(2 * n_parts):
        xs.append(step * (i + 1) + (i % 3))
    return lambda w: write_floor1(w, [0] * n_parts, {0: 2}, {0: 1}, {0: class_book}, {0: [sub_book, -1]}, 2, rangebits, xs)


def _ladder(a, b):
    return list(range(a, b + 1))


LONGCODE_NAMES = ("longcode_res1", "longcode_res2", "longcode_many_books")


def _longcode_config(name, books):
    """Setups whose codebooks libvorbis never writes (long, sparse, ordered, under-subscribed), one shape per route of the two
    parsers' symbol decode (host_setup.cpp: generate_table / Codebook::decode_scalar; nvh_setup.hip: upload_parse_tables).
    Stereo, blocks 256 / 2048.  DESIGN.md section 3 lists which book exists for which route; tests/test_long_codes.py asserts,
    through nvh_stream_parse_book_info, that each book takes it."""
    T2 = dict(lookup=2, min_me=(-9, -5), delta_me=(1, -4), value_bits=5)
    LAT = dict(lookup=1, min_me=(-4, -3), delta_me=(1, -2), value_bits=3)
    cls = VarBook([1, 3, 3, 4, 4, 5, 5, 6, 6, 11, 11, 12, 12, 12, 13, 13], dims=2)  # classbook: 16 words, 7 of them past the prefix
    fm = VarBook([1, 11, 12, 12])               # floor1 masterbook (under-subscribed)
    fs = VarBook([1, 11, 12, 12], "ordered")    # floor1 subclass book, written ordered (the reference's max_bits: 13)
    sparse_few = [0] * 64
    for k, n in enumerate(_ladder(1, 10) + [14, 14]):
        sparse_few[5 * k + 1] = n               # 12 of 64 used: stays sparse, entries reached through values[]
    sparse_many = [0] * 64
    for pos, n in zip([i for i in range(64) if i % 8 < 5], [2, 11, 3, 12, 13, 3, 4, 11, 4, 12] + [4, 5, 5, 5, 5, 13] + [11, 12, 13] * 8):
        sparse_many[pos] = n                    # 40 of 64 used: converted to dense, 24 entries stay unused
    if name == "longcode_res1":
        new = [cls, fm, fs,
               VarBook(_ladder(1, 30) + [31, 31], dims=2, **T2),                      # 14: the ladder, dense: max_bits 31
               VarBook([1] + [12] * 2048, dims=2, **T2),                              # 15: 512 groups of four codes
               VarBook(_ladder(1, 10) + [17] * 71, dims=2, **LAT),                    # 16: lattice 9 x 9, one group of 71
               VarBook(_ladder(1, 10) + [18] * 200, dims=2, **T2),                    # 17: one group of 200
               VarBook(_ladder(1, 10) + [18] * 256, dims=4, **T2),                    # 18: one group of 256
               VarBook(sparse_few, "sparse", dims=2, **LAT),                          # 19: lattice 8 x 8, sparse
               VarBook(sparse_many, "sparse", dims=2, **LAT),                         # 20: lattice 8 x 8, sparse -> dense
               VarBook(_ladder(1, 31) + [31], "ordered", dims=4, **T2)]               # 21: the ladder, ordered: max_bits 32
        floors = [_floor1_small(0, 1), _floor1_long(12, 13, 10)]
        residues = [lambda w: write_residue(w, 1, 0, 128, 16, 11, [1, 2, 7, 0], [14, 16, 17, 20, 19]),
                    lambda w: write_residue(w, 1, 8, 1000, 32, 11, [3, 5, 6, 7], [15, 21, 18, 17, 14, 16, 20, 19, 16])]
    elif name == "longcode_res2":
        sparse_t2 = [0] * 64
        for k, n in enumerate(_ladder(1, 9) + [12]):
            sparse_t2[6 * k + 2] = n
        new = [cls, fm, fs,
               VarBook([5] * 16 + [13] * 4096, dims=2, **T2),                         # 14: 4096 overflow nodes
               VarBook(_ladder(1, 12) + [24] * 16, dims=2, **T2),                     # 15: a group 14 bits deep
               VarBook(_ladder(1, 9) + (_ladder(11, 22) + [22]) * 2, dims=4, **T2),   # 16: two groups 12 bits deep
               VarBook(_ladder(1, 10) + [17] * 71, dims=4, **LAT),                    # 17: lattice 3^4
               VarBook(_ladder(1, 10) + [15] * 20, dims=3, **T2),                     # 18: dimension 3, explicit table
               VarBook(_ladder(1, 10) + [16] * 17, dims=3, **LAT),                    # 19: lattice 3^3
               VarBook(sparse_t2, "sparse", dims=2, **T2)]                            # 20: explicit table, sparse
        floors = [_floor1_small(12, 13), _floor1_long(0, 1, 10)]
        residues = [lambda w: write_residue(w, 2, 0, 200, 16, 11, [1, 2, 7, 0], [15, 17, 14, 16, 20]),
                    lambda w: write_residue(w, 2, 6, 1986, 36, 11, [3, 5, 6, 7], [18, 15, 19, 14, 16, 17, 18, 20, 19])]
    else:  # eighteen residue books with a 1024-slot prefix table each: 18 K words, the LDS image takes 16 K
        new = [VarBook(_ladder(1, 10) + [11, 11], dims=2, **T2) for _ in range(18)]  # 11 .. 28
        floors = [_floor1_small(0, 1), _floor1_long(0, 1, 10)]
        residues = [lambda w: write_residue(w, 1, 0, 128, 16, 2, [0x3F, 0x1F, 0x3F, 1], list(range(11, 29))),
                    lambda w: write_residue(w, 1, 8, 1000, 32, 2, [0xAA, 0x55, 3, 0], [28, 27, 26, 25, 24, 23, 22, 21, 12, 11])]
    return dict(books=books + new, channels=2, block0=256, block1=2048, floors=floors, residues=residues,
                mappings=[lambda w: write_mapping(w, 2, 1, [(0, 1)], None, [(0, 0)]),
                          lambda w: write_mapping(w, 2, 1, [(1, 0)], None, [(1, 1)])],
                modes=[(0, 0), (1, 1)])


BLOCK_SIZES = (64, 128, 256, 512, 1024, 2048, 4096, 8192)


def grid_name(ch, b0, b1):
    return "grid_%dch_%d_%d" % (ch, b0, b1)


def grid_cell(name):
    """(channels, block0, block1) of a grid name."""
    ch, b0, b1 = name[len("grid_"):].split("_")
    ch, b0, b1 = int(ch[:-2]), int(b0), int(b1)
    if ch not in (1, 2) or b0 not in BLOCK_SIZES or b1 not in BLOCK_SIZES or b0 > b1:
        raise KeyError(name)
    return ch, b0, b1


# every pair block0 <= block1 that Vorbis I allows, mono and stereo: 72 setups of one recipe (tests/test_block_grid.py).  Kept
# out of CONFIG_NAMES: the tests parametrised over that list would each grow by 72.
GRID_NAMES = [grid_name(ch, b0, b1) for ch in (1, 2) for b0 in BLOCK_SIZES for b1 in BLOCK_SIZES if b0 <= b1]


def _grid_config(name):
    """One recipe for every block-size pair: config()'s books; two Floor1 with X lists scaled to the block (two partitions below
    64 bins, else three for the short and five for the long block); a per-channel Residue1 over the whole short block; a long
    residue from bin 8 in partitions of 32 up to the last whole partition -- Residue1 for mono, a Residue2 over both channels for
    stereo --; stereo couples (0, 1) in short and (1, 0) in long blocks.  With block0 == block1 both modes stay: one frame size
    reached through either block flag."""
    ch, b0, b1 = grid_cell(name)

    def floor(n, long_block):
        half = n // 2
        return _floor1_long(0, 1, max(ilog(half - 1), 5), 2 if half < 64 else (5 if long_block else 3))

    ps0 = 8 if b0 // 2 < 64 else 16
    e0 = b0 // 2 // ps0 * ps0
    e1 = (b1 // 2 - 8) // 32 * 32 + 8
    rtype1, end1 = (1, e1) if ch == 1 else (2, 2 * e1 - 8)
    cpl = (lambda pair: []) if ch == 1 else (lambda pair: [pair])
    return dict(channels=ch, block0=b0, block1=b1,
                floors=[floor(b0, False), floor(b1, True)],
                residues=[lambda w: write_residue(w, 1, 0, e0, ps0, 2, [1, 2, 7, 0], [3, 4, 3, 4, 5]),
                          lambda w: write_residue(w, rtype1, 8, end1, 32, 2, [3, 1, 4, 6], [3, 4, 5, 5, 4, 3])],
                mappings=[lambda w: write_mapping(w, ch, 1, cpl((0, 1)), None, [(0, 0)]),
                          lambda w: write_mapping(w, ch, 1, cpl((1, 0)), None, [(1, 1)])],
                modes=[(0, 0), (1, 1)])


def config(name):
    # common books: 0 = 1-bit scalar (masterbook / class word helper), 1 = 2-bit scalar (floor posts 0..3),
    # 2 = 4-bit classbook (dim 2, 4 classes), 3 = VQ dim2 16 entries lattice, 4 = VQ dim4 256 entries lattice,
    # 5 = VQ dim8 256 entries lattice, 6 = VQ dim3 8 entries explicit (type 2), 7 = VQ dim2 sequence_p lattice,
    # 8 = VQ dim1 4 entries, 9 = VQ dim5 32 entries type 2
    books = [
        Book(1), Book(2), Book(4, dims=2),
        Book(4, dims=2, lookup=1, min_me=(-3, -2), delta_me=(1, -1), value_bits=3, mults=[0, 2, 4, 6]),
        Book(8, dims=4, lookup=1, min_me=(-5, -4), delta_me=(3, -4), value_bits=3, mults=[0, 1, 2, 3]),
        Book(8, dims=8, lookup=1, min_me=(-1, -3), delta_me=(1, -2), value_bits=2, mults=[0, 1]),
        Book(3, dims=3, lookup=2, min_me=(-7, -5), delta_me=(1, -4), value_bits=4),
        Book(4, dims=2, lookup=1, min_me=(-3, -3), delta_me=(1, -3), value_bits=3, sequence_p=1, mults=[1, 0, 3, 2]),
        Book(2, dims=1, lookup=1, min_me=(-3, -4), delta_me=(1, -3), value_bits=3, mults=[0, 2, 4, 6]),
        Book(5, dims=5, lookup=2, min_me=(-9, -6), delta_me=(1, -5), value_bits=5),
        # floor0 LSP book: dim 4, values in (0, pi): min 0.2, delta ~0.18
        Book(8, dims=4, lookup=1, min_me=(13, -6), delta_me=(45, -6), value_bits=2, mults=[0, 1, 2, 3]),
    ]
    c = dict(books=books, rate=44100)
    if name == "mono_res0_small_blocks":      # generic kernels (n < 256), Residue0, mono
        c.update(channels=1, block0=64, block1=128,
                 floors=[_floor1_small(0, 1)],
                 residues=[lambda w: write_residue(w, 0, 0, 64, 8, 2, [1, 3, 5, 0], [3, 3, 8, 3, 5])],
                 mappings=[lambda w: write_mapping(w, 1, 1, [], None, [(0, 0)])],
                 modes=[(0, 0), (1, 0)])
    elif name == "stereo_res1_coupled":       # Residue1 with two channels and coupling
        c.update(channels=2, block0=256, block1=2048,
                 floors=[_floor1_small(0, 1), _floor1_long(0, 1, 10)],
                 residues=[lambda w: write_residue(w, 1, 0, 128, 16, 2, [1, 2, 7, 0], [3, 4, 3, 4, 5]),
                           lambda w: write_residue(w, 1, 8, 1000, 32, 2, [3, 1, 4, 6], [3, 4, 5, 5, 4, 3])],
                 mappings=[lambda w: write_mapping(w, 2, 1, [(0, 1)], None, [(0, 0)]),
                           lambda w: write_mapping(w, 2, 1, [(1, 0)], None, [(1, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name == "three_ch_res2_misaligned":  # quirk B-1: partition size not a channel multiple, two coupling steps
        c.update(channels=3, block0=256, block1=1024,
                 floors=[_floor1_small(0, 1), _floor1_long(0, 1, 9)],
                 residues=[lambda w: write_residue(w, 2, 0, 360, 16, 2, [1, 3, 0, 2], [3, 4, 3, 3]),
                           lambda w: write_residue(w, 2, 4, 1500, 32, 2, [1, 3, 5, 2], [4, 3, 5, 3, 4, 5])],
                 mappings=[lambda w: write_mapping(w, 3, 1, [(0, 1), (2, 1)], None, [(0, 0)]),
                           lambda w: write_mapping(w, 3, 1, [(0, 2), (1, 2)], None, [(1, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name == "six_ch_res2_4096":          # BASELINE config C4 shape: 6 channels, n = 4096, psize 48
        c.update(channels=6, block0=512, block1=4096, rate=48000,
                 floors=[_floor1_small(0, 1), _floor1_long(0, 1, 11, n_parts=8)],
                 residues=[lambda w: write_residue(w, 2, 0, 6 * 200, 48, 2, [1, 3, 0, 2], [3, 4, 3, 3]),
                           lambda w: write_residue(w, 2, 0, 6 * 1536, 48, 2, [1, 3, 5, 7], [4, 3, 5, 3, 4, 5, 3, 4])],
                 mappings=[lambda w: write_mapping(w, 6, 1, [(0, 2), (3, 4)], None, [(0, 0)]),
                           lambda w: write_mapping(w, 6, 1, [(0, 2), (3, 4)], None, [(1, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name == "floor0_stereo":             # Floor0 (no shipped file uses it)
        c.update(channels=2, block0=256, block1=1024,
                 floors=[lambda w: write_floor0(w, 8, 22050, 64, 5, 40, [10]),
                         lambda w: write_floor0(w, 7, 22050, 128, 6, 30, [10])],
                 residues=[lambda w: write_residue(w, 1, 0, 128, 8, 2, [1, 1, 3, 0], [8, 3, 3, 4])],  # (short blocks: up to n/2)
                 mappings=[lambda w: write_mapping(w, 2, 1, [(0, 1)], None, [(0, 0)]),
                           lambda w: write_mapping(w, 2, 1, [], None, [(1, 0)])],
                 modes=[(0, 0), (1, 1)])
    elif name == "floor0_slab":               # Floor0 (even and odd order) and a Floor1 mode, residues the slab kernels take
        c.update(channels=2, block0=256, block1=2048,
                 floors=[lambda w: write_floor0(w, 8, 22050, 64, 5, 40, [10]),
                         lambda w: write_floor0(w, 7, 22050, 128, 6, 30, [10]),
                         _floor1_long(0, 1, 10)],
                 residues=[lambda w: write_residue(w, 2, 0, 200, 16, 2, [1, 2, 7, 0], [3, 4, 3, 4, 5]),
                           lambda w: write_residue(w, 2, 0, 1800, 32, 2, [3, 1, 4, 6], [3, 4, 5, 5, 4, 3])],
                 mappings=[lambda w: write_mapping(w, 2, 1, [(0, 1)], None, [(0, 0)]),
                           lambda w: write_mapping(w, 2, 1, [(1, 0)], None, [(1, 1)]),
                           lambda w: write_mapping(w, 2, 1, [(0, 1)], None, [(2, 1)])],
                 modes=[(0, 0), (1, 1), (1, 2)])
    elif name == "two_submaps":               # quirk B-3: every channel ends up ForceNoEnergy
        c.update(channels=2, block0=256, block1=512,
                 floors=[_floor1_small(0, 1), _floor1_small(0, 1)],
                 residues=[lambda w: write_residue(w, 1, 0, 100, 4, 2, [1, 1, 1, 0], [3, 8, 4]),
                           lambda w: write_residue(w, 0, 0, 100, 4, 2, [1, 1, 1, 0], [3, 3, 8])],
                 mappings=[lambda w: write_mapping(w, 2, 2, [(0, 1)], [0, 1], [(0, 0), (1, 1)])],
                 modes=[(0, 0), (1, 0)])
    elif name == "equal_blocks_overrun":      # block0 == block1; book dimension 3 / 5 does not divide the partition size
        c.update(channels=2, block0=1024, block1=1024,
                 floors=[_floor1_long(0, 1, 9)],
                 residues=[lambda w: write_residue(w, 1, 0, 400, 16, 2, [1, 2, 3, 0], [6, 9, 6, 7]),
                           lambda w: write_residue(w, 2, 0, 800, 16, 2, [1, 2, 3, 0], [6, 9, 7, 3])],
                 mappings=[lambda w: write_mapping(w, 2, 1, [(0, 1)], None, [(0, 0)]),
                           lambda w: write_mapping(w, 2, 1, [], None, [(0, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name == "mono_8192":                 # largest block size
        c.update(channels=1, block0=2048, block1=8192,
                 floors=[_floor1_long(0, 1, 11, n_parts=4), _floor1_long(0, 1, 13, n_parts=10)],
                 residues=[lambda w: write_residue(w, 1, 0, 900, 32, 2, [1, 3, 0, 2], [3, 4, 3, 3]),
                           lambda w: write_residue(w, 2, 0, 4000, 64, 2, [1, 3, 5, 7], [4, 3, 5, 3, 4, 5, 3, 4])],
                 mappings=[lambda w: write_mapping(w, 1, 1, [], None, [(0, 0)]),
                           lambda w: write_mapping(w, 1, 1, [], None, [(1, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name == "stereo_8192":               # largest block size, two coupled channels: the slab kernels' non-in-place transform
        c.update(channels=2, block0=512, block1=8192,
                 floors=[_floor1_long(0, 1, 9, n_parts=3), _floor1_long(0, 1, 13, n_parts=10)],
                 residues=[lambda w: write_residue(w, 1, 0, 240, 16, 2, [1, 3, 0, 2], [3, 4, 3, 3]),
                           lambda w: write_residue(w, 2, 0, 7936, 64, 2, [1, 3, 5, 7], [4, 3, 5, 3, 4, 5, 3, 4])],
                 mappings=[lambda w: write_mapping(w, 2, 1, [(1, 0)], None, [(0, 0)]),
                           lambda w: write_mapping(w, 2, 1, [(0, 1)], None, [(1, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name == "mono_res1_2048":            # mono through the slab kernels (blocks 256 / 2048): paired emission with one channel
        c.update(channels=1, block0=256, block1=2048,
                 floors=[_floor1_small(0, 1), _floor1_long(0, 1, 10)],
                 residues=[lambda w: write_residue(w, 1, 0, 128, 16, 2, [1, 2, 7, 0], [3, 4, 3, 4, 5]),
                           lambda w: write_residue(w, 1, 8, 1000, 32, 2, [3, 1, 4, 6], [3, 4, 5, 5, 4, 3])],
                 mappings=[lambda w: write_mapping(w, 1, 1, [], None, [(0, 0)]),
                           lambda w: write_mapping(w, 1, 1, [], None, [(1, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name in ("res0_slab", "odd_dims_slab", "res2_alias_stereo", "two_pass_slab", "res0_3ch"):
        # the slab kernels' general bin walk (kernels_synth.hip: residue_walk_general): Residue0; lattice books of dimension
        # 1 / 3 / 5; Residue2 over two channels whose partitions (15 components) share bins (quirk B-1); two residue passes
        # per frame (two submaps with the same floor and residue, so that quirk B-3 leaves the channels their energy)
        c["books"] = books + [
            Book(6, dims=3, lookup=1, min_me=(-4, -3), delta_me=(1, -2), value_bits=3, mults=[0, 1, 3, 5]),   # 11
            Book(5, dims=5, lookup=1, min_me=(-2, -3), delta_me=(3, -3), value_bits=2, mults=[0, 3]),         # 12
        ]
        if name in ("res0_slab", "res0_3ch"):  # (res0_3ch: the same through the wide kernel, k_synth8_g)
            res = [lambda w: write_residue(w, 0, 0, 120, 24, 2, [1, 2, 7, 0], [3, 11, 4, 5, 8]),
                   lambda w: write_residue(w, 0, 8, 992, 24, 2, [3, 1, 4, 6], [3, 4, 5, 5, 11, 8])]
        elif name == "odd_dims_slab":
            res = [lambda w: write_residue(w, 1, 0, 120, 15, 2, [1, 2, 7, 0], [8, 11, 12, 11, 8]),
                   lambda w: write_residue(w, 1, 5, 995, 30, 2, [3, 1, 4, 6], [11, 12, 8, 3, 12, 11])]
        elif name == "res2_alias_stereo":
            res = [lambda w: write_residue(w, 2, 3, 243, 15, 2, [1, 2, 7, 0], [8, 11, 12, 11, 8]),
                   lambda w: write_residue(w, 2, 9, 1989, 30, 2, [3, 1, 4, 6], [11, 12, 8, 3, 12, 11])]
        else:
            res = [lambda w: write_residue(w, 1, 0, 128, 16, 2, [1, 2, 7, 0], [3, 4, 3, 4, 5]),
                   lambda w: write_residue(w, 2, 0, 1800, 32, 2, [3, 1, 4, 6], [3, 4, 5, 5, 4, 3])]
        two = name == "two_pass_slab"
        nch = 3 if name == "res0_3ch" else 2
        c.update(channels=nch, block0=256, block1=2048,
                 floors=[_floor1_small(0, 1), _floor1_long(0, 1, 10)],
                 residues=res,
                 mappings=[lambda w: write_mapping(w, nch, 2 if two else 1, [(0, 1)], [0, 1] if two else None, [(0, 0)] * (2 if two else 1)),
                           lambda w: write_mapping(w, nch, 2 if two else 1, [(nch - 1, 0)], [1, 0] if two else None, [(1, 1)] * (2 if two else 1))],
                 modes=[(0, 0), (1, 1)])
    elif name in ("table_books_pair", "table_books_general", "table_books_b1"):
        # books with an explicit table -- lookup type 2 (books 6, 9) and type 1 with sequence_p (book 7), Codebook.cs:262-281 -- in
        # residues the slab kernels take (round 6: kernels_synth.hip: table_value): on the pair walk (even dimensions, a per-channel
        # Residue1 and a stereo Residue2), on the general bin walk (dimensions 3 and 5 dividing 15 / 30), on the quirk-B-1 bin walk
        # (three channels, partitions off the channel grid); every residue mixes them with lattice books
        c["books"] = books + [
            Book(6, dims=2, lookup=2, min_me=(-9, -5), delta_me=(1, -4), value_bits=5),                       # 11: type 2, dim 2
            Book(7, dims=4, lookup=2, min_me=(-11, -6), delta_me=(1, -5), value_bits=5, sequence_p=1),       # 12: type 2 + sequence_p, dim 4
        ]
        if name == "table_books_pair":
            nch, cpl = 2, [(0, 1)]
            res = [lambda w: write_residue(w, 1, 0, 128, 16, 2, [1, 2, 7, 0], [7, 11, 3, 12, 7]),
                   lambda w: write_residue(w, 2, 0, 1800, 32, 2, [3, 1, 4, 6], [11, 4, 7, 12, 5, 11])]
        elif name == "table_books_general":
            nch, cpl = 2, [(0, 1)]
            res = [lambda w: write_residue(w, 1, 0, 120, 15, 2, [1, 2, 7, 0], [6, 9, 6, 9, 6]),
                   lambda w: write_residue(w, 2, 6, 1986, 30, 2, [3, 1, 4, 6], [6, 7, 9, 3, 6, 9])]
        else:
            nch, cpl = 3, [(0, 1), (2, 1)]
            res = [lambda w: write_residue(w, 2, 0, 360, 16, 2, [1, 3, 0, 2], [7, 11, 3, 12]),
                   lambda w: write_residue(w, 2, 4, 1500, 32, 2, [1, 3, 5, 2], [11, 7, 12, 3, 4, 7])]
        c.update(channels=nch, block0=256, block1=1024 if nch == 3 else 2048,
                 floors=[_floor1_small(0, 1), _floor1_long(0, 1, 9 if nch == 3 else 10)],
                 residues=res,
                 mappings=[lambda w: write_mapping(w, nch, 1, cpl, None, [(0, 0)]),
                           lambda w: write_mapping(w, nch, 1, cpl[::-1] if nch == 3 else [(1, 0)], None, [(1, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name in ("ch4_res1", "ch5_res2", "ch7_res1", "ch8_res2"):   # the channel counts no other config has
        nch, rtype = int(name[2]), int(name[-1])
        couple = [(0, 1), (2, 3)] if nch == 4 else [(0, 2), (3, 4)] if nch == 5 else [(0, 1), (2, 3), (5, 6)] if nch == 7 else [(0, 7), (1, 6), (2, 5)]
        mult = nch if rtype == 2 else 1
        c.update(channels=nch, block0=256, block1=2048,
                 floors=[_floor1_small(0, 1), _floor1_long(0, 1, 10)],
                 residues=[lambda w: write_residue(w, rtype, 0, mult * 120, 16, 2, [1, 2, 7, 0], [3, 4, 3, 4, 5]),
                           lambda w: write_residue(w, rtype, 8 * mult, mult * 960, 32, 2, [3, 1, 4, 6], [3, 4, 5, 5, 4, 3])],
                 mappings=[lambda w: write_mapping(w, nch, 1, couple, None, [(0, 0)]),
                           lambda w: write_mapping(w, nch, 1, couple[::-1], None, [(1, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name == "ch9_res2":                  # nine channels: 4-bit coupling fields, a step that names channel 8; Residue2 with
        # partitions that are whole multiples of the channel count (18 / 36: no quirk B-1), books of dimension 1 / 2 / 4
        cpl = [(0, 8), (3, 4), (8, 5)]
        c.update(channels=9, block0=256, block1=2048,
                 floors=[_floor1_small(0, 1), _floor1_long(0, 1, 10)],
                 residues=[lambda w: write_residue(w, 2, 0, 9 * 96, 18, 2, [1, 2, 7, 0], [3, 8, 7, 3, 8]),
                           lambda w: write_residue(w, 2, 0, 9 * 480, 36, 2, [3, 1, 4, 6], [3, 4, 3, 4, 4, 3])],
                 mappings=[lambda w: write_mapping(w, 9, 1, cpl, None, [(0, 0)]),
                           lambda w: write_mapping(w, 9, 1, cpl[::-1], None, [(1, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name == "ch16_res1_4096":            # sixteen channels at n = 4096: 128 KiB of spectra per frame.  The long residue has a
        # dimension-3 book in 16-value partitions (vector overrun: nvh_setup.hip marks the residue sequential), so the spectra may
        # not take the 152 KB LDS window either and the frame goes to the global-memory kernels k_residue + k_couple_floor
        cpl = [(0, 15), (1, 14), (7, 8), (12, 3)]
        c.update(channels=16, block0=512, block1=4096, rate=48000,
                 floors=[_floor1_small(0, 1), _floor1_long(0, 1, 11, n_parts=8)],
                 residues=[lambda w: write_residue(w, 1, 0, 200, 16, 2, [1, 2, 7, 0], [3, 8, 7, 3, 8]),
                           lambda w: write_residue(w, 1, 8, 520, 16, 2, [3, 1, 4, 6], [3, 6, 4, 3, 6, 4])],
                 mappings=[lambda w: write_mapping(w, 16, 1, cpl, None, [(0, 0)]),
                           lambda w: write_mapping(w, 16, 1, cpl[::-1], None, [(1, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name == "ch40_res1":                 # forty channels: 6-bit coupling fields, steps across channel 32 (the frame's 32-bit
        # execute masks do not reach there: nvh_format.h NvhFrame), modest residue ends
        cpl = [(0, 39), (31, 32), (33, 5), (20, 35), (36, 37)]
        c.update(channels=40, block0=256, block1=512,
                 floors=[_floor1_small(0, 1), _floor1_long(0, 1, 8, n_parts=3)],
                 residues=[lambda w: write_residue(w, 1, 0, 64, 16, 2, [1, 2, 7, 0], [3, 8, 7, 3, 8]),
                           lambda w: write_residue(w, 1, 0, 160, 16, 2, [3, 1, 4, 6], [3, 4, 3, 4, 4, 3])],
                 mappings=[lambda w: write_mapping(w, 40, 1, cpl, None, [(0, 0)]),
                           lambda w: write_mapping(w, 40, 1, cpl[::-1], None, [(1, 1)])],
                 modes=[(0, 0), (1, 1)])
    elif name in LONGCODE_NAMES:
        c.update(_longcode_config(name, books))
    elif name.startswith("grid_"):
        c.update(_grid_config(name))
    else:
        raise KeyError(name)
    return c


CONFIG_NAMES = ["mono_res0_small_blocks", "stereo_res1_coupled", "three_ch_res2_misaligned", "six_ch_res2_4096",
                "floor0_stereo", "floor0_slab", "two_submaps", "equal_blocks_overrun", "mono_8192", "stereo_8192", "ch4_res1", "ch5_res2", "ch7_res1", "ch8_res2", "mono_res1_2048",
                "res0_slab", "odd_dims_slab", "res2_alias_stereo", "two_pass_slab", "res0_3ch",
                "table_books_pair", "table_books_general", "table_books_b1", "ch9_res2", "ch16_res1_4096", "ch40_res1"] + list(LONGCODE_NAMES)


def _residue_args(residue):
    """write_residue's arguments behind one of a configuration's residue writers, read back from the bits it writes."""
    w = BitWriter()
    residue(w)
    bits, pos = int.from_bytes(w.bytes(), "little"), [0]

    def rd(n):
        v = (bits >> pos[0]) & ((1 << n) - 1)
        pos[0] += n
        return v

    rtype, begin, end, psize, nclass, classbook = rd(16), rd(24), rd(24), rd(24) + 1, rd(6) + 1, rd(8)
    cascades = []
    for _ in range(nclass):
        low = rd(3)
        cascades.append(low | ((rd(5) if rd(1) else 0) << 3))
    books = [rd(8) for c in cascades for _ in range(bin(c).count("1"))]
    return rtype, begin, end, psize, classbook, cascades, books


ROUNDING_STAGES = 3
FLOOR0_LSP_BOOK = 10


def rounding(name):
    """config(name) with residue sums that round (tests/test_residue_rounding.py).  config()'s value books are dyadic with a
    mantissa of a few bits and most classes have at most two cascade stages: every partial sum is exact and two addends commute,
    so no order of additions can be told from another.  Here every class of every residue has three stages (cascade 7), its
    books taken cyclically from the residue's own list -- the dimensions and lookup types, and with them the kernel route, stay
    -- and every value book a residue uses gets a minimum and a delta with a full 21-bit mantissa, at a scale that changes by up
    to 2^15 from one book to the next: sums of three terms round, and the rounded sum depends on the order.  All values stay in
    the normal range.  The Floor0 LSP book keeps its values (its curves must stay bounded); multiplicands, entry counts,
    sequence_p and lookup types are config()'s.  Kept out of CONFIG_NAMES, as GRID_NAMES is."""
    import copy
    c = dict(config(name))
    books = list(c["books"])
    residues, used = [], set()
    for r in c["residues"]:
        rtype, begin, end, psize, classbook, cascades, rbooks = _residue_args(r)
        cyc = [rbooks[i % len(rbooks)] for i in range(ROUNDING_STAGES * len(cascades))]
        used.update(cyc)
        args = (rtype, begin, end, psize, classbook, [(1 << ROUNDING_STAGES) - 1] * len(cascades), cyc)
        residues.append(lambda w, args=args: write_residue(w, *args))
    for i in sorted(used):
        if books[i].lookup == 0 or i == FLOOR0_LSP_BOOK:
            continue
        books[i] = copy.copy(books[i])
        books[i].min_me = (-(0x155555 ^ (i * 0x1357)), -21 - 5 * (i % 4))
        books[i].delta_me = (0x1C71C7 ^ (i * 0x2461), -22 - 5 * (i % 4))
    c.update(books=books, residues=residues)
    return c


def filtered_stream(oracle, name, npackets, seed, consistent_windows=True):
    """make_stream, with every audio packet that makes the reference algorithm throw (a floor curve leaving the
    dB table) replaced by a fresh random one, so that the stream as a whole decodes."""
    import ctypes as C
    cfg = config(name)
    packets, gr, fl = make_stream(cfg, npackets, seed, consistent_windows)
    hdr = packets[:3]
    blob = b"".join(hdr)
    offs = np.zeros(4, np.int64)
    offs[1:] = np.cumsum([len(p) for p in hdr])
    g3 = np.full(3, -1, np.int64)
    f3 = np.zeros(3, np.uint8)
    bb = np.frombuffer(blob, dtype=np.uint8)
    err = C.c_int(0)
    d = oracle.L.orc_open_packets(bb.ctypes.data, offs.ctypes.data, g3.ctypes.data, f3.ctypes.data, 3, C.byref(err))
    assert d, "synthetic setup header rejected: %d" % err.value
    try:
        ch, b1 = oracle.L.orc_channels(d), oracle.L.orc_block1(d)
        planes = np.zeros(ch * b1, np.float32)
        a, b, c, e = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        rng = np.random.default_rng(seed + 99991)
        replaced = 0
        for i in range(3, len(packets)):
            for attempt in range(200):
                rc = oracle.L.orc_decode_packet_block(d, packets[i], len(packets[i]), planes.ctypes.data, C.byref(a), C.byref(b),
                                                      C.byref(c), C.byref(e))
                if rc >= 0 and np.isfinite(planes).all():
                    break
                head = packets[i][:1]
                body = rng.integers(0, 256, len(packets[i]) - 1).astype(np.uint8).tobytes()
                packets[i] = head + body
                replaced += 1
            else:
                raise AssertionError("could not find a decodable packet for " + name)
    finally:
        oracle.L.orc_close(d)
    return packets, gr, fl
