"""What tests/test_large_cpu.py and tests/test_gpu_large.py share: the shapes of the large calls ("Large calls").

Many rows: R = 65 601 rows whose content has the period 131 (row r carries row r mod 131 of a 131-row master), so that the
definition is evaluated for 131 rows only and a row index cut to 16 bits, or a row served by the wrong lap of a capped
grid, meets other content: 131 is prime, 65 536 mod 131 = 36 and R mod 131 = 101.

Far rows: a matrix of three rows (two of 8-byte elements) S = 2^31 + 24 elements apart, and S + 1 for the paths that leave
16-byte alignment, whose first row starts M = 2^31 + 8 elements into one device allocation, the arena.  The layout
arithmetic is plain integers and needs no GPU: `wrapped` lists where a row would land if its offset were cut to 32 bits
in any of four ways, and tests/test_large_cpu.py proves that every such place lies inside the arena and is not the true
one.  A kernel with such a cut therefore shows as wrong bits or a touched guard byte, never as a fault.  The arena itself
(`Arena`) needs torch and a GPU."""
import numpy as np

ROWS = 65601                    # R: past 2^16; no multiple of 16, 64 or 131
PERIOD = 131
STRIDE = 2 ** 31 + 24           # S, in elements; S + 1 leaves 16-byte alignment
MARGIN = 2 ** 31 + 8            # M: elements in front of row 0
TAIL = 4096                     # elements behind the last row's start (a row is shorter than this)
PATTERN = 0xA5                  # the guard byte: a negative normal float, -23131 as int16, no NaN under any view
MODES = ("u32 elements", "s32 elements", "u32 bytes", "s32 bytes")
CHUNK = 2 ** 28                 # bytes of the arena that one fill or one check touches


def far_rows(elem_size):
    """Rows of a far matrix: three, or two of 8-byte elements (row 1 then lies at 16 GiB)."""
    return 2 if elem_size == 8 else 3


def arena_elems(elem_size, stride=STRIDE + 1):
    """Elements of the arena for this element size: the margin, the rows at the larger of the two strides, a tail."""
    return MARGIN + (far_rows(elem_size) - 1) * stride + TAIL


def arena_bytes(elem_size):
    return arena_elems(elem_size) * elem_size


def row_start(r, stride):
    """Element of the arena at which row r starts."""
    return MARGIN + r * stride


def _cut(v, signed):
    v &= 0xFFFFFFFF
    return v - 2 ** 32 if signed and v >= 2 ** 31 else v


def wrapped(r, stride, elem_size):
    """{mode: byte of the arena at which row r would start if r * stride (or its byte count) were cut to 32 bits}"""
    base = MARGIN * elem_size
    off = r * stride
    return {"u32 elements": base + _cut(off, False) * elem_size, "s32 elements": base + _cut(off, True) * elem_size,
            "u32 bytes": base + _cut(off * elem_size, False), "s32 bytes": base + _cut(off * elem_size, True)}


def residues(rows=ROWS):
    """r mod 131 for r < rows: int64"""
    return np.arange(rows, dtype=np.int64) % PERIOD


def shuffled_map(rows=ROWS):
    """A row_map that keeps every row in its residue class and sends rows across 2^16: the blocks of 131 rows in reverse
    order (row 131 k + j reads row 131 (last - k) + j, `last` the last block that has a row j), a permutation."""
    r = np.arange(rows, dtype=np.int64)
    k, j = r // PERIOD, r % PERIOD
    last = (rows - 1 - j) // PERIOD
    m = PERIOD * (last - k) + j
    assert ((m % PERIOD) == j).all() and np.array_equal(np.sort(m), r) and m[:PERIOD].max() >= 2 ** 16 and m[2 ** 16:].max() < PERIOD
    return m


def pattern_word(dtype):
    """The guard as one element of a numpy dtype"""
    return np.frombuffer(bytes([PATTERN]) * np.dtype(dtype).itemsize, dtype)[0]


class Arena:
    """One device allocation that holds a far matrix of `elem_size`-byte elements at either stride.  fill(): every byte is
    PATTERN.  matrix(): the far matrix as a strided view.  dirty(): the bytes that are not PATTERN, counted on the device in
    chunks."""

    def __init__(self, torch, elem_size, device="cuda:0"):
        self.torch = torch
        self.elem_size = elem_size
        self.bytes = (arena_bytes(elem_size) + 7) // 8 * 8
        self.buf = torch.empty(self.bytes // 8, dtype=torch.int64, device=device)
        self.word = int(np.frombuffer(bytes([PATTERN]) * 8, np.int64)[0])

    def fill(self):
        step = CHUNK // 8
        for a in range(0, self.buf.numel(), step):
            self.buf[a:a + step].fill_(self.word)

    def matrix(self, dtype, n, stride, rows=None):
        flat = self.buf.view(dtype)
        assert flat.element_size() == self.elem_size
        rows = far_rows(self.elem_size) if rows is None else rows
        assert row_start(rows - 1, stride) + n <= flat.numel() and n <= TAIL
        return flat.as_strided((rows, n), (stride, 1), MARGIN)

    def erase(self, view):
        """the rows of a matrix() view back to the guard"""
        for r in range(view.shape[0]):
            row = self.torch.view_as_real(view[r]) if view.is_complex() else view[r]
            row.view(self.torch.uint8).fill_(PATTERN)

    def dirty(self):
        torch = self.torch
        step = CHUNK // 8
        bad = torch.zeros((), dtype=torch.int64, device=self.buf.device)
        for a in range(0, self.buf.numel(), step):
            bad += (self.buf[a:a + step] != self.word).sum()
        return int(bad)

    def free(self):
        self.buf = None
        self.torch.cuda.empty_cache()
