"""Reference model of fbk_bsi_moments (no GPU, no library): decode every column's value from the words, sum in Python ints,
reduce modulo 2^128.

    decode()      words of a fragment -> exists, magnitude, sign of every column (value = sign ? -magnitude : magnitude)
    brute()       the definition: a Python-int loop over the selected columns
    expected()    the same sums for whole shards: the magnitudes split into 16-bit limbs, the limb-pair sums in int64 (exact: a
                  product is below 2^32 and a call has fewer than 2^31 columns here), put together in Python ints
    chunk_bytes() / gram() / fold()   the arithmetic of the kernel: signed 7-bit chunk bytes, Gram matrix, fold (fbk_moments_plan.h)

tests/test_bsi_moments_cpu.py shows that the three agree; the GPU tests compare the library with expected()."""
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

import msum_ref as R

MASK128 = (1 << 128) - 1


class Moments(NamedTuple):
    n: int
    sum_x: int
    sum_y: int
    sum_xx: int
    sum_yy: int
    sum_xy: int


def wrap128(v: int) -> int:
    """v modulo 2^128 as a signed 128-bit integer"""
    v &= MASK128
    return v - (1 << 128) if v >> 127 else v


def wrapped(m: Moments) -> Moments:
    return Moments(m.n, *(wrap128(v) for v in m[1:]))


def decode(S: np.ndarray, depth: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """S [depth + 2, 16, 1024] uint64 -> (exists bool, magnitude uint64, negative bool), each [2^20].  Sign and plane bits
    outside exists are dropped; a set sign over magnitude 0 is the value 0 (negative is False there)."""
    b = R.bits(S)
    ex = b[0]
    mag = np.zeros(1 << 20, dtype=np.uint64)
    for k in range(depth):
        mag |= (b[2 + k] & ex).astype(np.uint64) << np.uint64(k)
    return ex, mag, b[1] & ex & (mag != 0)


def values_at(S: np.ndarray, depth: int, cols: Sequence[int]) -> List[Optional[int]]:
    """the stored value of the given columns as Python ints, None where the column does not exist"""
    ex, mag, neg = decode(S, depth)
    return [(-int(mag[c]) if neg[c] else int(mag[c])) if ex[c] else None for c in cols]


def brute(xs: Sequence[int], ys: Optional[Sequence[int]]) -> Moments:
    """xs, ys: the values of the selected columns (ys None: the one-field form)"""
    if ys is None:
        return wrapped(Moments(len(xs), sum(xs), 0, sum(x * x for x in xs), 0, 0))
    return wrapped(Moments(len(xs), sum(xs), sum(ys), sum(x * x for x in xs), sum(y * y for y in ys), sum(x * y for x, y in zip(xs, ys))))


def brute_shards(Sx: np.ndarray, dx: int, Sy: Optional[np.ndarray], dy: int, F: Optional[np.ndarray]) -> Moments:
    """the definition over whole shards ([n_shards, depth + 2, 16, 1024], F [n_shards, 16, 1024] or None): slow, for small E"""
    xs, ys = [], []
    for s in range(Sx.shape[0]):
        ex, mx, nx = decode(Sx[s], dx)
        sel = ex.copy()
        if Sy is not None:
            ey, my, ny = decode(Sy[s], dy)
            sel &= ey
        if F is not None:
            sel &= R.bits(F[s])
        cols = np.flatnonzero(sel)
        xs += [(-int(mx[c]) if nx[c] else int(mx[c])) for c in cols]
        if Sy is not None:
            ys += [(-int(my[c]) if ny[c] else int(my[c])) for c in cols]
    return brute(xs, ys if Sy is not None else None)


def _limbs(mag: np.ndarray, neg: np.ndarray) -> np.ndarray:
    """[4, n] int64: the 16-bit limbs of the magnitudes, each carrying the sign"""
    sgn = np.where(neg, -1, 1).astype(np.int64)
    return np.stack([((mag >> np.uint64(16 * i)) & np.uint64(0xFFFF)).astype(np.int64) * sgn for i in range(4)])


def expected_each(Sx: np.ndarray, dx: int, Sy: Optional[np.ndarray], dy: int, filters: Sequence[Optional[np.ndarray]],
                  ix: Optional[Sequence[int]] = None, iy: Optional[Sequence[int]] = None, ifl: Optional[Sequence[int]] = None) -> List[Moments]:
    """the moments for every filter of the list ([n, 16, 1024] or None: no filter) over the same fields, decoded once.
    ix / iy / ifl: shard s reads fragment ix[s] of Sx, iy[s] of Sy and row ifl[s] of every filter (base_rows may alias: a few
    distinct fragments serve many shards); None: shard s reads entry s."""
    n_sh = len(ix) if ix is not None else Sx.shape[0]
    ix = list(range(n_sh)) if ix is None else list(ix)
    iy = list(range(n_sh)) if iy is None else list(iy)
    ifl = list(range(n_sh)) if ifl is None else list(ifl)
    dec_x = {k: decode(Sx[k], dx) for k in sorted(set(ix))}
    dec_y = {k: decode(Sy[k], dy) for k in sorted(set(iy))} if Sy is not None else {}
    fbits = [{k: R.bits(F[k]) for k in sorted(set(ifl))} if F is not None else None for F in filters]
    n = [0] * len(filters)
    lin = [np.zeros((2, 4), dtype=object) for _ in filters]
    quad = [np.zeros((3, 4, 4), dtype=object) for _ in filters]  # xx, yy, xy
    times = {}  # shards that read the same (x, y, filter) fragments count once, times their number
    for s in range(n_sh):
        times[(ix[s], iy[s], ifl[s])] = times.get((ix[s], iy[s], ifl[s]), 0) + 1
    for (kx, ky, kf), mult in times.items():
        ex, mx, nx = dec_x[kx]
        both = ex
        if Sy is not None:
            ey, my, ny = dec_y[ky]
            both = ex & ey
        for k in range(len(filters)):
            sel = both & fbits[k][kf] if fbits[k] is not None else both
            n[k] += mult * int(sel.sum())
            lx = _limbs(mx[sel], nx[sel])
            ax = np.abs(lx)
            lin[k][0] += mult * lx.sum(axis=1).astype(object)
            quad[k][0] += mult * (ax @ ax.T).astype(object)
            if Sy is not None:
                ly = _limbs(my[sel], ny[sel])
                ay = np.abs(ly)
                lin[k][1] += mult * ly.sum(axis=1).astype(object)
                quad[k][1] += mult * (ay @ ay.T).astype(object)
                # x·y = sign_x sign_y |x| |y|: the sign once, on the x side
                quad[k][2] += mult * ((ax * np.where(nx[sel] ^ ny[sel], -1, 1)) @ ay.T).astype(object)
    put1 = lambda v: sum(int(v[i]) << (16 * i) for i in range(4))
    put2 = lambda m: sum(int(m[i, j]) << (16 * (i + j)) for i in range(4) for j in range(4))
    return [wrapped(Moments(n[k], put1(lin[k][0]), put1(lin[k][1]), put2(quad[k][0]), put2(quad[k][1]), put2(quad[k][2]))) for k in range(len(filters))]


def expected(Sx: np.ndarray, dx: int, Sy: Optional[np.ndarray], dy: int, F: Optional[np.ndarray]) -> Moments:
    return expected_each(Sx, dx, Sy, dy, [F])[0]


# ---- the kernel's arithmetic -------------------------------------------------------------------------------------------------------

def chunks_of(depth: int) -> int:
    return -(-depth // 7)


def rows_of(dx: int, dy: int) -> Tuple[int, int, int, int]:
    """(chunks of x, chunks of y, the mask's row, rows) of the byte matrix M"""
    cx, cy = chunks_of(dx), chunks_of(dy)
    return cx, cy, cx + cy, cx + cy + 1


def chunk_bytes(mag: np.ndarray, neg: np.ndarray, depth: int) -> np.ndarray:
    """[chunks, n] int8: chunk m = bits 7m .. 7m+6 of the magnitude, negated where the value is negative"""
    out = np.zeros((chunks_of(depth), mag.size), dtype=np.int8)
    for m in range(out.shape[0]):
        c = ((mag >> np.uint64(7 * m)) & np.uint64(0x7F)).astype(np.int16)
        out[m] = np.where(neg, -c, c).astype(np.int8)
    return out


def gram(mx, nx, dx: int, my, ny, dy: int) -> np.ndarray:
    """[32, 32] int64: G = M · Mᵀ over the given (already selected) columns"""
    cx, cy, mask, n_rows = rows_of(dx, dy)
    M = np.zeros((32, mx.size), dtype=np.int64)
    M[:cx] = chunk_bytes(mx, nx, dx)
    if cy:
        M[cx:mask] = chunk_bytes(my, ny, dy)
    M[mask] = 1
    return M @ M.T


def fold(S: np.ndarray, dx: int, dy: int) -> Moments:
    """fbk_moments_plan.h fold(): the chunk-pair sums -> moments, modulo 2^128"""
    cx, cy, mask, _ = rows_of(dx, dy)
    lin = lambda r0, n: sum(int(S[mask, r0 + m]) << (7 * m) for m in range(n))
    bil = lambda a0, na, b0, nb: sum(int(S[a0 + m, b0 + k]) << (7 * (m + k)) for m in range(na) for k in range(nb))
    return wrapped(Moments(int(S[mask, mask]), lin(0, cx), lin(cx, cy), bil(0, cx, 0, cx), bil(cx, cy, cx, cy), bil(0, cx, cx, cy)))


def densify_chunk(n_shards: int, x_dense: bool, dx: int, y_dense: Optional[bool], dy: int, f_dense: Optional[bool]) -> int:
    """the densify chunk of a call (include/fbk.h, fbk_bsi_moments); y_dense / f_dense None: the call has no y / no filter"""
    r = (0 if x_dense else dx + 2) + (0 if y_dense in (None, True) else dy + 2) + (0 if f_dense in (None, True) else 1)
    if r == 0 or n_shards == 0:
        return n_shards
    most = max(1, min(n_shards, (1 << 30) // ((1 << 17) * r)))
    passes = -(-n_shards // most)
    return -(-n_shards // passes)
