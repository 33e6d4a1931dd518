"""Hand-built LZ4 blocks for the two bitshuffle-LZ4 decoders (csrc/kernels_decode.hpp on the GPU, host/codecs.hpp on the host),
and the model they are judged by.

A plain helper module (no fixtures, no pytest settings).  It has
  * seq() / block(): LZ4 sequences with canonical length fields, so a test chooses the sequence structure itself;
  * decode(): an independent byte-by-byte model of the LZ4 block format that also says what each sequence looked like (how many
    extension bytes its two length fields had, where its token lay, how close the kernel's in-place literal copy came to its source);
  * chunk() / frame(): any block bytes are SOME frame -- the model's output through the inverse of bslz4.bitshuffle -- so the expected
    pixels need no encoder;
  * catalogue(): the cases, in three classes.
      A  conforming: the block ends with a literal-only sequence of at least 5 bytes and its last match starts at least 12 bytes
         before the end.  liblz4 accepts it; every decoder must give the model's bytes.
      B  lenient: liblz4 refuses the block (it ends on a match, or with fewer than 5 literals, or a match begins in the last 12
         bytes), the model and the host decoder decode it.  The GPU decoder may decode it (then to the model's bytes) or refuse it.
      C  malformed: the model gives None and every decoder must refuse.  Every class C input is rejected by a bounds check ON READING
         (each note names the line of kernels_decode.hpp that does); none is meant to make anything fault.

Random literal bytes come from a fixed seed and the case's name, so a case keeps its bytes when the catalogue around it changes.
"""
import os
import zlib
from collections import namedtuple

import numpy as np

BLOCK = 8192                 # kDecBlockBytes: bytes of a full block
PAYLOAD = BLOCK + 72         # kDecPayload: the kernel stages a block so that it ends here (aligned down to the block's offset mod 4)
MAX_CLEN = BLOCK + 64        # the longest block the kernel stages (line 142)
SHORT = {2: 48, 4: 64}       # bytes of the short last block of FRAMES, per element size
SEED = 0x124B10C5

# the smallest frames with a first, a middle and a last full block, a short block and a raw tail:
# u16 97 x 127 = 3 x 4096 + 24 + 7 (the odd width exercises put8's straddle branches), u32 61 x 101 = 3 x 2048 + 16 + 1
FRAMES = {"u16": (97, 127, np.uint16), "u32": (61, 101, np.uint32)}

LIT_EXT = (0, 1, 6, 7, 8, 9, 14, 15, 16, 17, 31, 32)     # the literal-length loop reloads its window after 7, 15, 23 and 31 bytes
MATCH_EXT = (0, 1, 5, 6, 7, 8, 13, 14, 15, 30, 31)       # the match-length loop after 6, 14, 22 and 30
OFFSETS = (1, 2, 3, 4, 7, 8, 63, 64, 65, 127, 128)       # (8187 cannot be conforming: see class B)
MLENS = (4, 5, 18, 19, 63, 64, 65, 128, 273, 274, 529)

Case = namedtuple("Case", "name cls cap data note")       # cap: the bytes the block must decode to
ChunkCase = namedtuple("ChunkCase", "name data match note")   # a whole chunk the host's planning or the kernel must refuse


def rnd(name, n):
    """n random bytes that depend on the seed and the name alone."""
    return np.random.default_rng([SEED, zlib.crc32(name.encode())]).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- sequence builder ------------------------------------------------------------------------------------------------

def _ext(v):
    """The extension bytes of a length field whose value (after the token's 15) is v - 15."""
    return b"\xff" * ((v - 15) // 255) + bytes([(v - 15) % 255])


def seq(literals=b"", offset=None, match_len=None):
    """One sequence: token, literal length, literals and -- unless it is the block's last -- offset and match length."""
    lit, ml = len(literals), 0 if offset is None else match_len - 4
    out = bytes([min(lit, 15) << 4 | min(ml, 15)]) + (_ext(lit) if lit >= 15 else b"") + literals
    if offset is not None:
        out += bytes([offset & 255, offset >> 8]) + (_ext(ml) if ml >= 15 else b"")
    return out


def block(*seqs):
    return b"".join(seqs)


# ---- the model ---------------------------------------------------------------------------------------------------------

def decode(src, cap, off=0):
    """(the cap bytes the block decodes to, or None when it is malformed; a dict per sequence).  off: the block's byte offset in the
    kernel's input, which decides where the kernel stages it.  A sequence's dict has at / match_at (bytes before its token / its
    offset field), op, lit, lit_ext, lit_last, distance (read position - write position when the kernel's in-place literal copy
    begins) and, with a match, offset, mlen, match_ext, match_last."""
    start = PAYLOAD - len(src) - (PAYLOAD - len(src) - off) % 4
    out, trace, i = bytearray(), [], 0

    def field(nibble):   # a length field: its value, extension bytes and last extension byte (None: the input ends inside it)
        nonlocal i
        value, n, last = nibble, 0, None
        while nibble == 15 and last in (None, 255):
            if i >= len(src):
                return None
            last = src[i]
            value, n, i = value + last, n + 1, i + 1
        return value, n, last

    while i < len(src):
        t = {"at": i, "op": len(out)}
        trace.append(t)
        token, i = src[i], i + 1
        if (f := field(token >> 4)) is None:
            return None, trace
        t["lit"], t["lit_ext"], t["lit_last"] = f
        t["distance"] = start + i - len(out)
        if i + f[0] > len(src) or len(out) + f[0] > cap:
            return None, trace
        out += src[i:i + f[0]]
        i += f[0]
        if i == len(src):
            break
        if i + 2 > len(src):
            return None, trace
        t["match_at"], t["offset"], i = i, src[i] | src[i + 1] << 8, i + 2
        if (f := field(token & 15)) is None:
            return None, trace
        t["mlen"], t["match_ext"], t["match_last"] = f[0] + 4, f[1], f[2]
        if not 0 < t["offset"] <= len(out) or len(out) + t["mlen"] > cap:
            return None, trace
        for _ in range(t["mlen"]):
            out.append(out[-t["offset"]])
    return (bytes(out) if len(out) == cap else None), trace


# ---- chunks and frames ---------------------------------------------------------------------------------------------------

def blocking(W, H, dtype):
    """(element size, full blocks, bytes of the short last block or 0, raw tail bytes) of a frame: bitshuffle's blocking."""
    es = np.dtype(dtype).itemsize
    n, per = W * H, BLOCK // es
    rem = n % per
    return es, n // per, rem // 8 * 8 * es, rem % 8 * es


def unshuffle(planes, dtype):
    """The inverse of bslz4.bitshuffle: es*8 bit planes -> the elements."""
    es = np.dtype(dtype).itemsize
    bits = np.unpackbits(np.frombuffer(planes, np.uint8).reshape(es * 8, -1), axis=1, bitorder="little")   # [byte*8+bit][elem]
    elems = np.packbits(bits.reshape(es, 8, -1).transpose(2, 0, 1), axis=2, bitorder="little")             # [elem][byte][1]
    return np.ascontiguousarray(elems.reshape(-1, es)).view(dtype).reshape(-1)


def chunk(W, H, dtype, payloads, tail, total=None):
    """The 12-byte header, a big-endian length and the payload per block, the raw tail."""
    es = np.dtype(dtype).itemsize
    out = (W * H * es if total is None else total).to_bytes(8, "big") + BLOCK.to_bytes(4, "big")
    return out + b"".join(len(p).to_bytes(4, "big") + p for p in payloads) + tail


def frame(W, H, dtype, outputs, tail):
    """The frame a chunk stands for: what its blocks decode to, un-shuffled, then the tail."""
    parts = [unshuffle(o, dtype) for o in outputs] + [np.frombuffer(tail, dtype)]
    return np.concatenate(parts).reshape(H, W)


# ---- the catalogue ---------------------------------------------------------------------------------------------------------

def _rest(name, used, cap=BLOCK):
    """Completes a block whose sequences so far decode to `used` bytes, with nothing a case is about: sequences of 100 literals and a
    match of 100 at offset 100 (length fields of one byte, the plain copy), then a last run of 13 to 212 literals (fewer when fewer
    are left)."""
    out, left, k = [], cap - used, 0
    while left > 212:
        out.append(seq(rnd(f"{name}/rest{k}", 100), 100, 100))
        left, k = left - 200, k + 1
    return block(*out, seq(rnd(name + "/rest", left)))


def _lead(name, p):
    """An earlier sequence of p (mod 4) bytes, so that the next token's address takes that residue: p + 5 literals, a match of 4 (plain copy)."""
    return seq(rnd(name + "/lead", p + 5), 4, 4), p + 9


def _class_a():
    c = []

    def add(name, data, note, cap=BLOCK):
        c.append(Case(name, "A", cap, data, note))

    # literal-length fields of n extension bytes whose last is r, the token at address p (mod 4)
    for n in LIT_EXT:
        for r in ((0, 1, 254) if n else (1, 14)):
            for p in range(4):
                name = f"lit_ext{n}_r{r}_p{p}"
                L = 15 + 255 * (n - 1) + r if n else r
                lead, used = _lead(name, p)
                if BLOCK - used - L >= 20:     # the run, a match of 4 that reads its end, the rest
                    data = block(lead, seq(rnd(name, L), 4, 4), _rest(name, used + L + 4))
                else:                          # the run is the block's last sequence: a longer match ahead of it makes up the size
                    nl = next(k for k in range(2, 14) if (3 + k + (len(_ext(BLOCK - L - k - 4)) if BLOCK - L - k >= 19 else 0)) % 4 == p)
                    data = block(seq(rnd(name + "/lead", nl), nl, BLOCK - L - nl), seq(rnd(name, L)))
                add(name, data, f"literal run of {L}: {n} extension bytes, the last {r if n else '-'}; token at {p} mod 4")
    # match-length fields, the same way (3 literals ahead of the offset keep the field's address at the token's residue)
    for n in MATCH_EXT:
        for r in ((0, 1, 254) if n else (0, 14)):
            for p in range(4):
                name = f"match_ext{n}_r{r}_p{p}"
                M = 19 + 255 * (n - 1) + r if n else 4 + r
                lead, used = _lead(name, p)
                add(name, block(lead, seq(rnd(name, 3), 3, M), _rest(name, used + 3 + M)),
                    f"match of {M}: {n} extension bytes, the last {r if n else '-'}; token and offset field at {p} mod 4")
    # offsets x lengths: the three copy loops (offset >= mlen plain, offset 1 broadcast, else modulo)
    for o in OFFSETS:
        for m in MLENS:
            name = f"match_off{o}_len{m}"
            add(name, block(seq(rnd(name, o + 9), o, m), _rest(name, o + 9 + m)), f"offset {o}, length {m}, behind {o + 9} literals")
    for m in (4, 5, 19, 64, 65, 128, 274):
        for o in (m - 1, m, m + 1):
            name = f"border_len{m}_off{o}"
            add(name, block(seq(rnd(name, o + 2), o, m), _rest(name, o + 2 + m)), f"offset - length = {o - m}: the border between the plain and the modulo copy")
    for k, m in ((1, 4), (4, 64), (64, 65), (200, 529), (8180, 4)):
        name = f"match_offop{k}_len{m}"
        add(name, block(seq(rnd(name, k), k, m), _rest(name, k + m)), f"offset == op == {k}: the match reads the whole output so far")
    name = "fresh_literals"
    add(name, block(seq(rnd(name, 200), 200, 200), _rest(name, 400)), "a match that reads all the bytes this sequence's literals just wrote (the barrier ahead of the match copy)")
    name = "prev_match_tail"
    add(name, block(seq(rnd(name, 40), 40, 40), seq(b"", 8, 100), seq(rnd(name + "/2", 3), 64, 64), _rest(name, 247)),
        "a match that reads the last 8 bytes of the match before it, then one that reads that match's last 61")
    name = "back_to_back"
    add(name, block(seq(rnd(name, 20), 20, 20), seq(b"", 7, 33), seq(b"", 33, 33), _rest(name, 106)), "two matches with no literals between them")
    # the in-place margin.  The kernel stages a block of clen bytes so that it ends at PAYLOAD - a (a < 4: alignment); a literal copy then
    # reads `distance` = 72 - a + (output still to come) - (input still to come) bytes above where it writes.
    for X in (4, 19, 274, 529, 4096, 8000, 8179):
        name = f"head_tail_{X}"
        add(name, block(seq(rnd(name, 1), 1, X), seq(rnd(name + "/tail", BLOCK - 1 - X))),
            f"1 literal, a match of {X} at offset 1, {BLOCK - 1 - X} literals: the block's last run always copies over 72 - a bytes")
    # ... so a run comes closer only when input longer than its output follows it: a last run whose length field has e bytes
    for e in (32, 12, 10, 9, 8, 7, 6, 1):
        for R in (192, 193, 194, 195):
            name = f"head_run{R}_tail_e{e}"
            L = 15 + 255 * (e - 1)
            X = BLOCK - 1 - R - 4 - L
            add(name, block(seq(rnd(name, 1), 1, X), seq(rnd(name + "/run", R), 7, 4), seq(rnd(name + "/tail", L))),
                f"1 literal, a match of {X}, a run of {R} literals copied over {73 - e} - a bytes, a match of 4, a last run with {e} length bytes")
    add("max_expansion", block(seq(b"\xa5", 1, 8186), seq(rnd("max_expansion", 5))), "1 literal, a match of 8186, 5 literals: 43 bytes")
    name = "min_gain"
    add(name, block(seq(rnd(name, 4), 4, 4), seq(b"", 4, 4) * 2044, _rest(name, 8184)), "2045 matches of 4 with no literals behind a 4-byte head, 8 literals")
    name = "seqs_1634"
    add(name, block(*[seq(rnd(f"{name}/{k}", 1), 1 + k % 5, 4) for k in range(1634)], _rest(name, 8170)),
        "1634 sequences of 1 literal and a match of 4, 22 literals (conforming: liblz4 accepts it)")
    # sizes
    add("literals_only", seq(rnd("literals_only", BLOCK)), "one run of 8192 literals: 8226 bytes")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_real_encoder_block.bin"), "rb") as f:
        add("real_encoder", f.read(), "a block liblz4 wrote: bit planes of 4096 noisy 16-bit pixels with a few spots")
    for cap in SHORT.values():
        add(f"short{cap}_literals", seq(rnd(f"short{cap}", cap)), f"a short last block of {cap} bytes, literals only", cap)
        add(f"short{cap}_match", block(seq(b"\x5a", 1, cap - 13), seq(rnd(f"short{cap}m", 12))), f"a short last block: 1 literal, a match of {cap - 13}, 12 literals", cap)
    return c


def _class_b():
    c = []

    def add(name, data, note):
        c.append(Case(name, "B", BLOCK, data, note))
    name = "ends_on_match"
    add(name, seq(rnd(name, 8000), 100, 192), "the block ends exactly on a match")
    for k in range(5):
        name = f"final_literals_{k}"
        add(name, block(seq(rnd(name, 100), 50, BLOCK - 100 - k), seq(rnd(name + "/rest", k))), f"a final literal run of {k} bytes")
    name = "match_in_last_12"
    add(name, block(seq(rnd(name, 8181), 3, 6), _rest(name, 8187)), "the last match starts 11 bytes before the end")
    # the largest offset a conforming block can hold is 8180 (class A's match_offop8180_len4): a match must start 12 bytes before the end
    for m in (4, 5):
        name = f"match_off8187_len{m}"
        add(name, block(seq(rnd(name, 8187), 8187, m), *([_rest(name, 8187 + m)] if m == 4 else [])),
            f"offset 8187 == op, length {m}: " + ("1 final literal" if m == 4 else "ends on the match"))
    return c


def _class_c():
    c = []
    good = block(seq(rnd("c/good", 100), 10, 50))     # 100 literals and a match of 50: otherwise-valid surroundings

    def add(name, data, note, cap=BLOCK):
        c.append(Case(name, "C", cap, data, note))
    for name, o, note in (("offset_0", 0, "offset 0"), ("offset_op_plus_1", 101, "offset op + 1"), ("offset_ffff_op100", 0xFFFF, "offset 0xFFFF at op = 100")):
        add(name, block(seq(rnd(name, 100), o, 50), _rest(name, 150)), note + ": line 202 (offset == 0 || offset > op)")
    add("match_overruns_block_1", seq(rnd("mo", 100), 10, BLOCK - 99), "a match that ends 1 byte past the block: line 202 (op + mlen > out_bytes)")
    add("literals_overrun_input_1", block(good, _rest("li", 150)[:-1]), "a literal run 1 byte longer than the input: line 181 (pos + lit > end)")
    add("literals_overrun_output_1", block(good, seq(rnd("lo", BLOCK - 149))), "a literal run that ends 1 byte past the block: line 181 (op + lit > out_bytes)")
    add("literals_overrun_output_1_alone", seq(rnd("loa", BLOCK + 1)), "8193 literals and nothing else, 8227 bytes: line 181 (op + lit > out_bytes)")
    add("lit_field_unterminated", block(good, b"\xf0" + b"\xff" * 20),
        "a literal-length field of 0xFF bytes up to the block's end: line 176, or line 181 where the byte behind the block is not 0xFF")
    add("lit_field_unterminated_longest", b"\xf0" + b"\xff" * (MAX_CLEN - 1),
        "the same as the whole of the longest block the kernel stages (8256 bytes, 1032 window reloads): line 176 or 181")
    add("match_field_unterminated", block(good, bytes([0xAF]) + rnd("mu", 10) + b"\x0a\x00" + b"\xff" * 20),
        "a match-length field of 0xFF bytes up to the block's end: line 198, or line 202 (pos > end) where the byte behind the block is not 0xFF")
    add("ends_inside_offset", block(good, bytes([0x20]) + rnd("eo", 2) + b"\x01"), "the input ends after one offset byte: line 202 (pos > end)")
    add("output_1_short", block(good, _rest("os", 151)), "a well-formed block that decodes to 8191 bytes: line 219 (op != out_bytes)")
    add("extra_byte", block(good, _rest("eb", 150), b"\x10"), "a valid block and one more byte: the block's last run is then followed by half an offset: line 202 (pos > end)")
    for cap in SHORT.values():     # short last blocks: the bytes behind them are the tail's, which the GPU test makes 0xFF
        for k in (4, 5, 6, 7):
            add(f"short{cap}_lit_field_unterminated_{k}", b"\xf0" + b"\xff" * k,
                "a literal-length field that runs into the 0xFF tail: line 176 where the block does not end on a dword of the input, else 181", cap)
            add(f"short{cap}_match_field_unterminated_{k}", b"\x1f\x77\x01\x00" + b"\xff" * k,
                "a match-length field that runs into the 0xFF tail: line 198 where the block does not end on a dword of the input, else 202", cap)
    return c


_catalogue = None


def catalogue():
    global _catalogue
    if _catalogue is None:
        _catalogue = _class_a() + _class_b() + _class_c()
        assert len({c.name for c in _catalogue}) == len(_catalogue)
    return _catalogue


_decoded = {}


def decoded(case):
    """decode() of a case at offset 0, computed once (the model is slow) and never changed."""
    if case.name not in _decoded:
        _decoded[case.name] = decode(case.data, case.cap)
    return _decoded[case.name]


_fillers = []


def fillers():
    """Class A blocks of 8192 bytes whose compressed length is 0, 1, 2 and 3 mod 4: the blocks around a case in a chunk, which move the
    case's byte offset over all four residues."""
    if _fillers:
        return _fillers
    out = {}
    for k in range(4):
        name = f"filler{k}"
        data = block(seq(rnd(name, 20), 8, 4), seq(b"", 8, 4) * k, _rest(name, 24 + 4 * k))     # (a match of 4 takes a byte less than 4 literals)
        out[len(data) % 4] = Case(name, "A", BLOCK, data, f"filler of {len(data)} bytes")
    assert sorted(out) == [0, 1, 2, 3]
    _fillers.extend(out[k] for k in range(4))
    return _fillers


_elements = {}


def chunk_with(key, case=None, position=1, residue=0):
    """A chunk of FRAMES[key] and the frame it stands for (None when `case` is malformed).  `case` is full block `position`, or the
    short last block when that is its size; the other full blocks are fillers, the one ahead of the case chosen so that the case's
    payload begins at `residue` mod 4 in the chunk (block 0 always begins at 0); the short block is literals and the tail is 0xFF.
    -> (chunk, frame, the residue the case got)"""
    W, H, dtype = FRAMES[key]
    es, n_full, short, tail_bytes = blocking(W, H, dtype)
    fill = fillers()
    blocks = [fill[(k + residue) % 4] for k in range(n_full)] + [Case(f"chunk_short{short}", "A", short, seq(rnd("chunk/short", short)), "")]
    if case is not None:
        if case.cap == short:
            position = n_full
        assert case.cap == blocks[position].cap, (case.name, key)
        blocks[position] = case
        if position:
            before = sum(len(b.data) for b in blocks[:position - 1])
            blocks[position - 1] = fill[(residue - before) % 4]
    got = sum(len(b.data) for b in blocks[:position]) % 4
    tail = b"\xff" * tail_bytes
    payloads = [b.data for b in blocks]
    if any(decoded(b)[0] is None for b in blocks):
        return chunk(W, H, dtype, payloads, tail), None, got
    for b in blocks:     # (a block's elements are computed once per element type)
        if (b.name, key) not in _elements:
            _elements[b.name, key] = unshuffle(decoded(b)[0], dtype)
    elems = np.concatenate([_elements[b.name, key] for b in blocks] + [np.frombuffer(tail, dtype)])
    return chunk(W, H, dtype, payloads, tail), elems.reshape(H, W), got


def cases_for(key, cls):
    """The catalogue's cases of a class that fit FRAMES[key]: full blocks and that frame's short block."""
    sizes = (BLOCK, SHORT[np.dtype(FRAMES[key][2]).itemsize])
    return [c for c in catalogue() if c.cls == cls and c.cap in sizes]


def chunk_cases(key):
    """Whole chunks for FRAMES[key] that must be refused: by the kernel at its first check (line 142) or by the host's planning.
    match: the word the refusal must contain."""
    W, H, dtype = FRAMES[key]
    es, n_full, short, tail_bytes = blocking(W, H, dtype)
    good = chunk_with(key)[0]
    sizes = [int.from_bytes(good[12:16], "big")]
    at = [12]                                           # where the blocks' length prefixes lie
    for _ in range(n_full):
        at.append(at[-1] + 4 + sizes[-1])
        sizes.append(int.from_bytes(good[at[-1]:at[-1] + 4], "big"))
    payload = [good[a + 4:a + 4 + n] for a, n in zip(at, sizes)]
    tail = good[len(good) - tail_bytes:]
    with_block_1 = lambda b: chunk(W, H, dtype, [payload[0], b] + payload[2:], tail)
    return [ChunkCase("prefix_0", with_block_1(b""), "corrupt", "a block length prefix of 0: line 142"),
            ChunkCase("prefix_8257", with_block_1(seq(rnd("chunk/8257", BLOCK)) + b"\x10" * 31), "corrupt", "a block length prefix of kDecBlockBytes + 65: line 142"),
            ChunkCase("tail_cut_short", good[:-1], "run past", "the raw tail is 1 byte shorter than the frame needs: the host's planning refuses"),
            ChunkCase("prefixes_run_past", good[:12] + len(good).to_bytes(4, "big") + good[16:], "run past",
                      "the first block's length prefix is the whole chunk's size: the host's planning refuses"),
            ChunkCase("last_prefix_runs_past", good[:at[-1]] + (sizes[-1] + tail_bytes + 1).to_bytes(4, "big") + good[at[-1] + 4:], "run past",
                      "the last block's length prefix ends 1 byte behind the chunk: the host's planning refuses"),
            ChunkCase("header_size", chunk(W, H, dtype, payload, tail, total=W * H * es + 1), "header", "the header's frame size is off by one: chunk_ok refuses")]


if __name__ == "__main__":   # writes the one fixture the catalogue reads: a block from the real encoder (needs liblz4)
    import ctypes
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fast-feedback-service_amd", "python"))
    from ffs_amd import bslz4
    rng = np.random.default_rng(SEED)
    px = rng.poisson(3.0, 4096).astype(np.uint16)
    px[rng.integers(0, 4096, 40)] += rng.integers(100, 60000, 40).astype(np.uint16)
    planes = bslz4.bitshuffle(px)
    lib = bslz4.liblz4()
    dst = ctypes.create_string_buffer(lib.LZ4_compressBound(len(planes)))
    n = lib.LZ4_compress_default(planes, dst, len(planes), len(dst))
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_real_encoder_block.bin"), "wb") as f:
        f.write(dst.raw[:n])
    print(n, "bytes")
