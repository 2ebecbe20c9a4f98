"""Plain numpy / Python reference of the PNG encoder defined in include/instantavatar_hip_png.h ("PNG encoding"):
the filter choice, the tokens, the code construction, the block headers, the bit packing, the stored fallback, the Adler combination
and the PNG / APNG framing.  No GPU, no product import.  Written from the definition and from RFC 1950 / 1951 / the PNG and APNG
specifications, not from the kernels: the length-code table is the RFC's table (the kernels compute it arithmetically), the bit
writer is a Python integer, the Huffman merge runs on Python lists."""
import functools
import struct
import zlib

import numpy as np

DEFAULT_STRIP_ROWS = 16
MAX_STRIP_BYTES = 126976
ADLER = 65521
STORED_MAX = 65535
# RFC 1951 section 3.2.5: (code, extra bits, first length)
LENGTH_CODES = [(257, 0, 3), (258, 0, 4), (259, 0, 5), (260, 0, 6), (261, 0, 7), (262, 0, 8), (263, 0, 9), (264, 0, 10), (265, 1, 11),
                (266, 1, 13), (267, 1, 15), (268, 1, 17), (269, 2, 19), (270, 2, 23), (271, 2, 27), (272, 2, 31), (273, 3, 35), (274, 3, 43),
                (275, 3, 51), (276, 3, 59), (277, 4, 67), (278, 4, 83), (279, 4, 99), (280, 4, 115), (281, 5, 131), (282, 5, 163),
                (283, 5, 195), (284, 5, 227), (285, 0, 258)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}


def length_code(length):
    """match length 3 .. 258 -> (symbol, extra bits, extra value)"""
    assert 3 <= length <= 258
    for code, eb, first in reversed(LENGTH_CODES):
        if length >= first:
            if code == 285 or length < first + (1 << eb):
                return code, eb, length - first
    raise AssertionError(length)


# ---- filter ------------------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    a, b, c = a.astype(np.int32), b.astype(np.int32), c.astype(np.int32)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_image(img, swap_rb=False):
    """img [H,W,C] uint8 -> (filtered [H, 1 + W*C] uint8 with the type byte in front, types [H]).  The row above row 0 is zero; the type
    is the one of the smallest sum of |filtered byte read as int8|, a tie goes to the lower type."""
    img = np.asarray(img, np.uint8)
    H, W, C = img.shape
    if swap_rb:
        img = img[..., [2, 1, 0] + list(range(3, C))]
    raw = img.reshape(H, W * C).astype(np.int32)
    out = np.zeros((H, 1 + W * C), np.uint8)
    types = np.zeros(H, np.int64)
    zero = np.zeros(W * C, np.int32)
    for y in range(H):
        cur = raw[y]
        up = raw[y - 1] if y else zero
        left = np.concatenate([zero[:C], cur[:-C]]) if W * C > C else zero[:W * C].copy()
        upleft = np.concatenate([zero[:C], up[:-C]]) if W * C > C else zero[:W * C].copy()
        cands = [cur, cur - left, cur - up, cur - (left + up) // 2, cur - _paeth(left, up, upleft)]
        cands = [(c & 255).astype(np.uint8) for c in cands]
        costs = [int(np.abs(c.view(np.int8).astype(np.int32)).sum()) for c in cands]
        t = int(np.argmin(costs))          # (argmin: the first of equal minima = the lower type)
        types[y] = t
        out[y, 0] = t
        out[y, 1:] = cands[t]
    return out, types


# ---- tokens ------------------------------------------------------------------------------------------------------------------------------
def strip_tokens(s):
    """bytes of one strip -> list of tokens: ("L", byte) or ("M", length), every match at distance 1.  A maximal run of m + 1 equal bytes
    is one literal, floor(m / 258) matches of 258, then the remainder r as one match (r >= 3) or r literals."""
    s = np.asarray(s, np.uint8)
    heads = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    ends = np.concatenate([heads[1:], [len(s)]])
    toks = []
    for p, e in zip(heads.tolist(), ends.tolist()):
        v = int(s[p])
        toks.append(("L", v))
        m = e - p - 1
        toks.extend([("M", 258)] * (m // 258))
        r = m % 258
        if r >= 3:
            toks.append(("M", r))
        else:
            toks.extend([("L", v)] * r)
    return toks


# ---- code construction -------------------------------------------------------------------------------------------------------------------
def build_lengths(freq, limit, stats=None):
    """Code lengths of the symbols of `freq` (0 = unused, length 0), at most `limit` bits, Kraft sum exactly 1.  At least two used symbols.
      order   the used symbols ascending by (frequency, symbol)
      merge   Huffman's, on two queues (the leaves in that order, the merged nodes in the order they were made); of a leaf and a merged
              node of equal weight the leaf is taken first
      limit   n[d] = leaves of depth d; depths above the limit count as the limit; while the Kraft sum (in units of 2^-limit) exceeds
              2^limit: n[limit] -= 1, the deepest d < limit with n[d] > 0 gives n[d] -= 1, n[d + 1] += 2, and the sum drops by one
      hand    lengths 1, 2, ... are handed out from the END of the order (the most frequent symbol, the highest on a tie, first)"""
    used = sorted((f, s) for s, f in enumerate(freq) if f > 0)
    u = len(used)
    assert u >= 2
    w = [f for f, _ in used]
    iw, leaf_parent, int_parent = [], [0] * u, [0] * (u - 1)
    li = ii = 0
    for ni in range(u - 1):
        tot = 0
        for _ in range(2):
            if li < u and (ii >= len(iw) or w[li] <= iw[ii]):
                tot += w[li]
                leaf_parent[li] = ni
                li += 1
            else:
                tot += iw[ii]
                int_parent[ii] = ni
                ii += 1
        iw.append(tot)
    idepth = [0] * (u - 1)
    for k in range(u - 3, -1, -1):
        idepth[k] = idepth[int_parent[k]] + 1
    if stats is not None:
        stats["depth"] = max(stats.get("depth", 0), max(idepth[p] + 1 for p in leaf_parent))
    n = [0] * (limit + 1)
    for k in range(u):
        n[min(idepth[leaf_parent[k]] + 1, limit)] += 1
    total = sum(n[d] << (limit - d) for d in range(1, limit + 1))
    while total > (1 << limit):
        n[limit] -= 1
        for d in range(limit - 1, 0, -1):
            if n[d]:
                n[d] -= 1
                n[d + 1] += 2
                break
        total -= 1
    assert total == 1 << limit
    lens = [0] * len(freq)
    j = u
    for d in range(1, limit + 1):
        for _ in range(n[d]):
            j -= 1
            lens[used[j][1]] = d
    assert j == 0
    return lens


def canonical_codes(lens):
    """RFC 1951 section 3.2.2 -> the codes, MSB first"""
    mx = max(lens)
    bl = [0] * (mx + 2)
    for l in lens:
        if l:
            bl[l] += 1
    nxt, code = [0] * (mx + 2), 0
    for b in range(1, mx + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def kraft(lens):
    """sum of 2^-len over the used symbols as an exact fraction (numerator over 2^max)"""
    mx = max(lens)
    return sum(1 << (mx - l) for l in lens if l), 1 << mx


def code_length_tokens(seq):
    """the code lengths of both alphabets in one sequence -> [(symbol 0 .. 18, extra value)].  A maximal run of n equal values v (runs
    cross the boundary of the two alphabets):  v = 0: while n >= 11 one symbol 18 for min(n, 138); then one 17 if n >= 3, else n
    zeros.  v > 0: v once, then while n >= 3 one symbol 16 for min(n, 6), then the remaining n (0 .. 2) as v."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        n = j - i
        if v == 0:
            while n >= 11:
                c = min(n, 138)
                out.append((18, c - 11))
                n -= c
            if n >= 3:
                out.append((17, n - 3))
                n = 0
            out.extend([(0, 0)] * n)
        else:
            out.append((v, 0))
            n -= 1
            while n >= 3:
                c = min(n, 6)
                out.append((16, c - 3))
                n -= c
            out.extend([(v, 0)] * n)
        i = j
    return out


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, bits):          # LSB first
        assert 0 <= value < (1 << bits) or bits == 0
        self.acc |= value << self.n
        self.n += bits

    def put_code(self, code, length):    # Huffman codes go MSB first
        self.put(int(format(code, "0%db" % length)[::-1], 2), length)

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def stored_strip(s, last):
    out = bytearray()
    s = bytes(s)
    blocks = [s[i:i + STORED_MAX] for i in range(0, len(s), STORED_MAX)]
    for k, b in enumerate(blocks):
        out += bytes([1 if (last and k == len(blocks) - 1) else 0]) + struct.pack("<HH", len(b), len(b) ^ 0xFFFF) + b
    return bytes(out)


def stored_bytes(L):
    return L + 5 * ((L + STORED_MAX - 1) // STORED_MAX)


def encode_strip(s, last):
    """bytes of one strip -> (its piece of the zlib stream, "stored" | "dynamic", details)"""
    s = np.asarray(s, np.uint8)
    toks = strip_tokens(s)
    freq = [0] * 286
    for k, v in toks:
        freq[v if k == "L" else length_code(v)[0]] += 1
    freq[256] = 1
    st_ll, st_cl = {}, {}
    ll = build_lengths(freq, 15, st_ll)
    dl = [1, 1]                                        # the distance alphabet is always codes 0 and 1, one bit each
    hlit = max(257, max(i for i, l in enumerate(ll) if l) + 1)
    cl_toks = code_length_tokens(ll[:hlit] + dl)
    cf = [0] * 19
    for sym, _ in cl_toks:
        cf[sym] += 1
    cl = build_lengths(cf, 7, st_cl)
    hclen = max(4, max(i for i, sym in enumerate(CL_ORDER) if cl[sym]) + 1)
    llc, clc = canonical_codes(ll), canonical_codes(cl)
    w = BitWriter()
    w.put(1 if last else 0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(1, 5)                                        # HDIST - 1
    w.put(hclen - 4, 4)
    for sym in CL_ORDER[:hclen]:
        w.put(cl[sym], 3)
    for sym, ex in cl_toks:
        w.put_code(clc[sym], cl[sym])
        if sym in CL_EXTRA:
            w.put(ex, CL_EXTRA[sym])
    for k, v in toks:
        if k == "L":
            w.put_code(llc[v], ll[v])
        else:
            code, eb, ex = length_code(v)
            w.put_code(llc[code], ll[code])
            w.put(ex, eb)
            w.put(0, 1)                                # distance code 0 (distance 1), one bit, no extra bits
    w.put_code(llc[256], ll[256])
    if not last:                                       # sync flush: the empty stored block
        w.put(0, 3)
        w.align()
        w.put(0xFFFF0000, 32)
    coded = w.bytes()
    info = dict(ll=ll, cl=cl, ll_depth=st_ll["depth"], cl_depth=st_cl["depth"], hlit=hlit, hclen=hclen, tokens=len(toks), coded_bytes=len(coded))
    if len(coded) > stored_bytes(len(s)):
        return stored_strip(s, last), "stored", info
    return coded, "dynamic", info


def adler_combine(parts):
    """parts: (A = sum of bytes, B = sum of (len - i) * byte[i], len) per strip -> Adler-32 of the concatenation"""
    a, b = 1, 0
    for A, B, L in parts:
        b = (b + L * a + B) % ADLER
        a = (a + A) % ADLER
    return (b << 16) | a


def strip_sums(s):
    s = np.asarray(s, np.uint8).astype(np.int64)
    L = len(s)
    return int(s.sum()) % ADLER, int(((L - np.arange(L)) * s).sum()) % ADLER, L


def check_strip_rows(H, W, C, strip_rows):
    return C in (3, 4) and H >= 1 and W >= 1 and strip_rows >= 1 and min(strip_rows, H) * (W * C + 1) <= MAX_STRIP_BYTES


def encode_stream(img, swap_rb=False, strip_rows=DEFAULT_STRIP_ROWS):
    """img [H,W,C] uint8 -> (zlib stream, kinds per strip, details per strip, filtered bytes)"""
    img = np.asarray(img, np.uint8)
    H, W, C = img.shape
    assert check_strip_rows(H, W, C, strip_rows)
    filt, _ = filter_image(img, swap_rb)
    out, kinds, infos, sums = bytearray(b"\x78\x01"), [], [], []
    for r0 in range(0, H, strip_rows):
        s = filt[r0:r0 + strip_rows].reshape(-1)
        piece, kind, info = encode_strip(s, r0 + strip_rows >= H)
        out += piece
        kinds.append(kind)
        infos.append(info)
        sums.append(strip_sums(s))
    out += struct.pack(">I", adler_combine(sums))
    return bytes(out), kinds, infos, filt.tobytes()


def bound_bytes(n, H, W, C, strip_rows):
    if n < 0 or not check_strip_rows(H, W, C, strip_rows):
        return 0
    row = W * C + 1
    full, rest = divmod(H, strip_rows)
    per = 6 + full * stored_bytes(strip_rows * row) + (stored_bytes(rest * row) if rest else 0)
    return n * per


# ---- framing -----------------------------------------------------------------------------------------------------------------------------
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def ihdr(H, W, C):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, {3: 2, 4: 6}[C], 0, 0, 0))


def png_bytes(stream, H, W, C):
    return SIGNATURE + ihdr(H, W, C) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")


def apng_bytes(streams, H, W, C, fps=30, loop=0):
    """full-size frames, dispose none (0), blend source (0); the delay is 1 / fps as the fraction 1 over fps when fps is an integer"""
    num, den = delay_fraction(fps)
    out = bytearray(SIGNATURE + ihdr(H, W, C) + chunk(b"acTL", struct.pack(">II", len(streams), loop)))
    seq = 0
    for i, s in enumerate(streams):
        out += chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, num, den, 0, 0))
        seq += 1
        if i == 0:
            out += chunk(b"IDAT", s)
        else:
            out += chunk(b"fdAT", struct.pack(">I", seq) + s)
            seq += 1
    return bytes(out + chunk(b"IEND", b""))


def delay_fraction(fps):
    """frame delay 1 / fps seconds as 16-bit numerator and denominator: 1 / fps for an integer fps up to 65535, else round(1000 / fps) / 1000"""
    if float(fps) == int(fps) and 1 <= int(fps) <= 65535:
        return 1, int(fps)
    return max(1, min(65535, int(round(1000.0 / float(fps))))), 1000


# ---- the test cases shared by the CPU and the GPU tests ----------------------------------------------------------------------------------
SHAPES = [(1, 1, 4), (5, 7, 4), (5, 7, 3), (33, 19, 4)]
RUN_LENGTHS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 600)


def avatar_frame(size=64, seed=0):
    """a shaded ellipse with noise of one grey level on a transparent background: the kind of picture the renderer writes"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    u, v = (x - size / 2 + 0.5) / (size * 0.22), (y - size / 2 + 0.5) / (size * 0.42)
    inside = u * u + v * v <= 1.0
    shade = np.clip(200 - 90 * (u * 0.6 + v * 0.4), 0, 254)
    img = np.zeros((size, size, 4), np.uint8)
    for c, k in enumerate((1.0, 0.8, 0.6)):
        img[..., c] = np.where(inside, (shade * k).astype(np.int64) + g.integers(0, 2, (size, size)), 0)
    img[..., 3] = np.where(inside, 255, 0)
    return img


def runs_image(H, W, C):
    """rows built from runs of the lengths RUN_LENGTHS, every run of another value than its neighbours"""
    n = H * W * C
    out, v, k = [], 1, 0
    while sum(map(len, out)) < n:
        out.append(np.full(RUN_LENGTHS[k % len(RUN_LENGTHS)], v, np.uint8))
        v = v % 250 + 7
        k += 1
    return np.concatenate(out)[:n].reshape(H, W, C)


def fibonacci_image(H, W, C):
    """shuffled byte values with frequencies a[k + 1] = a[0] + ... + a[k - 1] + 3 (Fibonacci's growth: every merged node of Huffman's
    algorithm pairs with the next leaf), as many as fit: a tree deeper than the 15-bit limit.  The most frequent value is 0, then 1, -1,
    2, -2, ... as signed bytes, so that filter type 0 (the raw bytes) is the cheapest and the histogram survives the filter"""
    n = H * W * C
    w = [1, 2]
    while sum(w) + sum(w[:-1]) + 3 <= n:
        w.append(sum(w[:-1]) + 3)
    w = w[::-1]                            # rank 0 = the most frequent
    vals = np.concatenate([np.full(f, ((r + 1) // 2 if r % 2 else -(r // 2)) & 255, np.uint8) for r, f in enumerate(w)])
    vals = np.concatenate([vals, (40 + np.arange(n - len(vals)) % 2).astype(np.uint8)])       # (the rest: two values of one weight)
    np.random.default_rng(3).shuffle(vals)
    vals = vals.tolist()
    for i in range(2, n):                  # no three equal neighbours, so no matches: the next other value is swapped in
        if vals[i] == vals[i - 1] == vals[i - 2]:
            j = next((j for j in range(i + 1, n) if vals[j] != vals[i]), None)
            if j is not None:
                vals[i], vals[j] = vals[j], vals[i]
    return np.array(vals, np.uint8).reshape(H, W, C)


def contents(H, W, C):
    """{name: image [H,W,C]} of the issue's contents at one shape"""
    g = np.random.default_rng(1000 * H + 10 * W + C)
    yy, xx = np.mgrid[0:H, 0:W]
    disc = np.zeros((H, W, C), np.uint8)
    inside = (yy - (H - 1) / 2.0) ** 2 * W * W + (xx - (W - 1) / 2.0) ** 2 * H * H <= 0.16 * H * H * W * W
    disc[inside] = [200, 120, 40, 255][:C]
    across = np.zeros((H, W, C), np.uint8)         # zeros before and behind every strip boundary: the run of the filtered bytes goes on
    across[0, 0, 0] = 9                            # across it, and the first byte of a strip still has to be a literal
    return {
        "zeros": np.zeros((H, W, C), np.uint8),
        "constant": np.full((H, W, C), 37, np.uint8),
        "hramp": np.broadcast_to((np.arange(W, dtype=np.int64)[None, :, None] * 3 + np.arange(C)[None, None, :]) & 255, (H, W, C)).astype(np.uint8),
        "vramp": np.broadcast_to((np.arange(H, dtype=np.int64)[:, None, None] * 5) & 255, (H, W, C)).astype(np.uint8),
        "disc": disc,
        "runs": runs_image(H, W, C),
        "across": across,
        "random": g.integers(0, 256, (H, W, C), dtype=np.uint8),
    }


NOT_STORED = ("zeros", "constant", "hramp", "vramp", "disc")      # n_stored must be 0 for these (and for the avatar frame)


def strip_heights(H):
    return sorted({2, 16, H})


@functools.lru_cache(maxsize=None)
def case(shape, name, swap_rb, strip_rows):
    """the reference's result for one image, computed once and shared: (image, stream, kinds, infos, filtered)"""
    if name == "avatar":
        img = avatar_frame(shape[0])
    elif name == "fibonacci":
        img = fibonacci_image(*shape)
    else:
        img = contents(*shape)[name]
    img.setflags(write=False)
    return (img,) + encode_stream(img, swap_rb, strip_rows)


def all_cases():
    """(shape, content name) of every case of the issue, the avatar frame and the deep-tree case included"""
    out = [(s, n) for s in SHAPES for n in contents(*s)]
    return out + [((64, 64, 4), "avatar"), ((128, 128, 4), "fibonacci")]
