"""CBF byte-offset compression (cbfread.hpp:49-106; host/codecs.hpp has the C++ statement): a frame is the chain of its
pixels' deltas, each in 1, 3 or 7 bytes.  compress() is the encoder of the tests and tools, decompress() a plain reference
decoder; the product path decodes on the GPU (csrc/kernels_byteoffset.hpp)."""
import numpy as np


def compress(frame) -> bytes:
    """Shortest form per delta, the rule of byte_offset_compress: |d| <= 127 one byte; |d| <= 32767 0x80 + int16 (little-endian);
    otherwise 0x80 0x00 0x80 + the low 32 bits of d.  The values are taken as int32 (uint32 pixels by their bit pattern)."""
    a = np.asarray(frame)
    if a.dtype.kind == "u" and a.dtype.itemsize == 4:
        a = a.view(np.int32)
    v = a.astype(np.int32).reshape(-1).astype(np.int64)
    n = v.size
    if n == 0:
        return b""
    d = np.diff(v, prepend=np.int64(0))
    size = np.where(np.abs(d) <= 127, 1, np.where(np.abs(d) <= 32767, 3, 7))
    start = np.cumsum(size) - size
    out = np.zeros(int(start[-1] + size[-1]), np.uint8)
    u = (d & 0xFFFFFFFF).astype(np.uint64)
    one, three, seven = size == 1, size == 3, size == 7
    out[start[one]] = (u[one] & 0xFF).astype(np.uint8)
    s3 = start[three]
    out[s3] = 0x80
    out[s3 + 1] = (u[three] & 0xFF).astype(np.uint8)
    out[s3 + 2] = ((u[three] >> np.uint64(8)) & 0xFF).astype(np.uint8)
    s7 = start[seven]
    out[s7] = 0x80
    out[s7 + 2] = 0x80   # (out[s7 + 1] stays 0x00)
    for b in range(4):
        out[s7 + 3 + b] = ((u[seven] >> np.uint64(8 * b)) & 0xFF).astype(np.uint8)
    return out.tobytes()


def decompress(buf, n: int, dtype=np.int32) -> np.ndarray:
    """The first n elements of a byte-offset stream, truncated to dtype; fewer if the stream ends first (a token whose bytes run
    past the end emits nothing).  `current` accumulates modulo 2^32."""
    b = bytes(buf)
    out = np.zeros(n, np.uint32)
    cur, j, k, end = 0, 0, 0, len(b)
    while j < end and k < n:
        c = b[j]
        if c != 0x80:
            cur += c - 256 if c >= 128 else c
            j += 1
        else:
            if j + 3 > end:
                break
            s = b[j + 1] | (b[j + 2] << 8)
            if s != 0x8000:
                cur += s - 65536 if s >= 32768 else s
                j += 3
            else:
                if j + 7 > end:
                    break
                cur += int.from_bytes(b[j + 3:j + 7], "little")
                j += 7
        cur &= 0xFFFFFFFF
        out[k] = cur
        k += 1
    dt = np.dtype(dtype)
    return out[:k].astype(np.dtype(f"u{dt.itemsize}")).view(dt)
