"""Reference model of fbk_bsi_compare (no GPU, no library).

    definition()        decode every participating column to a Python int, add the base, compare: the meaning of the call
    sign_magnitude()    numpy model of the kernel's k == 0 instance, plane by plane on packed words
    general()           numpy model of the general instance: both streams into two's complement, k added bit by bit
    expected()          (lt, gt, E) words of whole shards by the instance the library takes; combine() applies an operator

tests/test_bsi_compare_cpu.py shows that the two recurrences equal the definition; the GPU tests compare the library with them.
Fragments are [depth + 2, 16, 1024] uint64 (row 0 exists, 1 sign, 2 + i plane i), as tests/moments_ref.py has them."""
from typing import Optional, Tuple

import numpy as np

import moments_ref as M
import msum_ref as R

EQ, NEQ, LT, LTE, GT, GTE = 1, 2, 3, 4, 5, 6
OPS = (EQ, NEQ, LT, LTE, GT, GTE)
PATH_OFFSET = 0x100
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def bitlen(k: int) -> int:
    return abs(k).bit_length()


def is_general(k: int, flags: int = 0) -> bool:
    return k != 0 or bool(flags & PATH_OFFSET)


def steps(dx: int, dy: int, k: int, flags: int = 0) -> int:
    """fbk_compare_plan.h steps(): W0 for the sign-magnitude instance, W = max(dx, dy, bitlen |k|) + 2 for the general one"""
    return max(dx, dy, bitlen(k)) + 2 if is_general(k, flags) else max(dx, dy)


def kbit(k: int, i: int) -> int:
    """bit i of k in two's complement, sign-extended (Python's >> on a negative int is arithmetic)"""
    return (k >> i) & 1


def definition(Sx: np.ndarray, dx: int, base_x: int, Sy: np.ndarray, dy: int, base_y: int,
               F: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(lt, gt, E) as bool [2^20]: E = exists_x & exists_y & F; lt / gt where value_x < / > value_y as exact integers.  A Python
    loop over the columns of E: for small E."""
    ex, mx, nx = M.decode(Sx, dx)
    ey, my, ny = M.decode(Sy, dy)
    E = ex & ey
    if F is not None:
        E = E & R.bits(F)
    lt, gt = np.zeros(1 << 20, dtype=bool), np.zeros(1 << 20, dtype=bool)
    for c in np.flatnonzero(E):
        vx = (-int(mx[c]) if nx[c] else int(mx[c])) + base_x
        vy = (-int(my[c]) if ny[c] else int(my[c])) + base_y
        lt[c], gt[c] = vx < vy, vx > vy
    return lt, gt, E


def _plane(S: np.ndarray, depth: int, i: int) -> np.ndarray:
    return S[2 + i] if i < depth else np.zeros((16, 1024), dtype=np.uint64)


def _participating(Sx, Sy, F):
    E = Sx[0] & Sy[0]
    return E & F if F is not None else E


def sign_magnitude(Sx: np.ndarray, dx: int, Sy: np.ndarray, dy: int, F: Optional[np.ndarray] = None):
    """k == 0: LSB -> MSB over the magnitude planes, then the signs; (lt, gt, E) words [16, 1024], lt / gt masked by E"""
    lt = np.zeros((16, 1024), dtype=np.uint64)
    gt, nz = lt.copy(), lt.copy()
    for i in range(max(dx, dy)):
        a, b = _plane(Sx, dx, i), _plane(Sy, dy, i)
        d = a ^ b
        lt = (~a & b) | (~d & lt)
        gt = (a & ~b) | (~d & gt)
        nz |= a | b
    sx, sy = Sx[1], Sy[1]
    flt = (sx & ~sy & nz) | (~sx & ~sy & lt) | (sx & sy & gt)
    fgt = (sy & ~sx & nz) | (~sx & ~sy & gt) | (sx & sy & lt)
    E = _participating(Sx, Sy, F)
    return flt & E, fgt & E, E


def general(Sx: np.ndarray, dx: int, Sy: np.ndarray, dy: int, k: int, F: Optional[np.ndarray] = None, width: Optional[int] = None):
    """any k: X = ±mx + k and Y = ±my streamed as `width`-bit two's complement numbers (default: the plan's W) and compared as
    signed numbers, a and b exchanged at the sign bit; carries out of the last step are dropped"""
    W = steps(dx, dy, k, PATH_OFFSET) if width is None else width
    sx, sy = Sx[1], Sy[1]
    cx, cy = sx.copy(), sy.copy()
    ck = np.zeros((16, 1024), dtype=np.uint64)
    lt, gt = ck.copy(), ck.copy()
    for i in range(W):
        ax, ay = _plane(Sx, dx, i) ^ sx, _plane(Sy, dy, i) ^ sy
        t = ax ^ cx
        cx = cx & ax
        b = ay ^ cy
        cy = cy & ay
        if kbit(k, i):
            a = ~(t ^ ck)
            ck = ck | t
        else:
            a = t ^ ck
            ck = ck & t
        if i == W - 1:
            a, b = b, a
        d = a ^ b
        lt = (~a & b) | (~d & lt)
        gt = (a & ~b) | (~d & gt)
    E = _participating(Sx, Sy, F)
    return lt & E, gt & E, E


def expected(Sx: np.ndarray, dx: int, base_x: int, Sy: np.ndarray, dy: int, base_y: int, F: Optional[np.ndarray] = None, flags: int = 0):
    """(lt, gt, E) words of one shard through the recurrence of the instance the library takes for these bases and flags"""
    k = base_x - base_y
    return general(Sx, dx, Sy, dy, k, F) if is_general(k, flags) else sign_magnitude(Sx, dx, Sy, dy, F)


def combine(op: int, lt: np.ndarray, gt: np.ndarray, E: np.ndarray) -> np.ndarray:
    """the operator's row from lt / gt / E (words or bools)"""
    if op == LT:
        return lt & E
    if op == GT:
        return gt & E
    if op == NEQ:
        return (lt | gt) & E
    if op == EQ:
        return E & ~(lt | gt)
    if op == LTE:
        return E & ~gt
    if op == GTE:
        return E & ~lt
    raise ValueError(op)


def words_of_bits(b: np.ndarray) -> np.ndarray:
    """bool [2^20] -> [16, 1024] uint64"""
    return np.packbits(b, bitorder="little").view(np.uint64).reshape(16, 1024)


def popcount(w: np.ndarray) -> int:
    return int(np.unpackbits(np.ascontiguousarray(w).view(np.uint8)).sum())
