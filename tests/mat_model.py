"""A numpy model of DspMat's "movers" -- the operations whose result is a bit-exact rearrangement of their input
(copies, zeros, sign flips) -- written from the docstrings in basic_dsp_amd/matrix.py as index arithmetic only: it never
calls the library.  MatModel / VecModel answer the same methods with the same signatures and codes as DspMat / DspVec,
so one driver (apply_step) runs a step on either; tests/test_mat_model.py pins every mover against oracle_lib and
tests/test_gpu_mat_sequences.py runs generated mover sequences on the GPU against the model, bit for bit.

The model also keeps the allocation's capacity by the library's rule (a buffer that is too small grows to
n + n / 8 + 64 scalars and never shrinks).  The capacity decides nothing in the model; it tells the sequence generator
and the dirty-state recipes which calls reallocate and when rows x row_len fills the allocation exactly.
"""
import numpy as np

TIME, FREQ = 0, 1
PAD_END, PAD_SURROUND, PAD_CENTER = 0, 1, 2
MAX_SCALARS = 1 << 20
STEPS = 16

# every DspMat operation that only moves scalars (or flips a sign, or writes zeros)
MOVERS = ("transpose", "zero_pad", "swap_halves", "fft_shift", "ifft_shift", "reverse", "zero_interleave", "decimatei",
          "mirror", "conj", "to_complex", "to_real", "to_imag", "get_real", "get_imag", "get_real_imag", "set_real_imag",
          "get_row", "set_row", "to_interleaved", "from_interleaved", "overlap_add", "from_frames", "from_vectors")


def grown_cap(n):
    """what a buffer that must hold n scalars and is too small grows to"""
    return n + n // 8 + 64


def _flip_sign(a):
    """-a as a flip of the sign bit: -0.0 <-> +0.0, and a NaN keeps its payload"""
    a = np.ascontiguousarray(a)
    u = a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
    return (u ^ (u.dtype.type(1) << u.dtype.type(8 * a.itemsize - 1))).view(a.dtype)


class VecModel:
    def __init__(self, a, is_complex=False, domain=TIME, delta=1.0):
        self.a = np.array(a, copy=True).reshape(-1)
        self._complex, self._domain = bool(is_complex), int(domain)
        self._delta = float(self.a.dtype.type(delta))

    def data(self):
        return self.a.copy()

    def __len__(self):
        return self.a.size

    def points(self):
        return self.a.size // (2 if self._complex else 1)

    def is_complex(self):
        return self._complex

    def domain(self):
        return self._domain

    def delta(self):
        return self._delta


class MatModel:
    def __init__(self, rows_data, is_complex=False, domain=TIME, delta=1.0):
        a = np.array(rows_data, copy=True)
        assert a.ndim == 2 and a.dtype in (np.float32, np.float64)
        assert not (is_complex and a.shape[1] % 2), "complex rows need an even scalar length"
        self.dtype = a.dtype.type
        self._complex, self._domain = bool(is_complex), int(domain)
        self._delta = float(self.dtype(delta))
        self.poisoned = False
        self._rows = a.shape[0]
        self.a = a if a.shape[0] else a.reshape(0, 0)   # a matrix without rows reports rows of length 0
        self.cap = grown_cap(max(a.size, 1))
        self.reallocs = 0                               # reallocations by calls, after the constructor's allocation

    # ------------------------------------------------------------------ metadata, as DspMat
    def rows(self):
        return self._rows

    def row_len(self):
        return self.a.shape[1] if self._rows else 0

    def row_points(self):
        return self.row_len() // self._e()

    def is_complex(self):
        return self._complex

    def domain(self):
        return self._domain

    def delta(self):
        return self._delta

    def data(self):
        return self.a.copy()

    # ------------------------------------------------------------------ helpers
    def _e(self):
        return 2 if self._complex else 1

    def _el(self):
        """[rows, points, e]: the scalars of one point stay together"""
        return self.a.reshape(self._rows, self.row_points(), self._e())

    def _put(self, a, rows=None):
        self._rows = a.shape[0] if rows is None else rows
        self.a = np.ascontiguousarray(a).reshape(self._rows, -1) if self._rows else np.zeros((0, 0), self.dtype)

    def _reserve(self, n):
        if n > self.cap:
            self.cap = grown_cap(n)
            self.reallocs += 1

    def _ret(self, code=0):
        return -1 if code == 0 and self.poisoned else code

    def _poison(self):
        self._put(np.zeros((self._rows, 0), self.dtype), self._rows)
        self._delta, self.poisoned = float("nan"), True
        return -1

    # ------------------------------------------------------------------ movers, in place
    def transpose(self):
        if self.poisoned:
            return -1
        if self._rows == 0 or self.row_points() == 0:
            self._put(np.zeros((0, 0), self.dtype))
            return 0
        self._put(self._el().transpose(1, 0, 2).reshape(self.row_points(), -1))
        return 0

    def zero_pad(self, points, option=PAD_END):
        e, pb = self._e(), self.row_points()
        if points * e <= self.row_len():
            return 7   # an argument error comes first
        if self.poisoned:
            return -1
        self._reserve(self._rows * points * e)
        out = np.zeros((self._rows, points, e), self.dtype)
        el = self._el()
        if option == PAD_END:
            out[:, :pb] = el
        elif option == PAD_SURROUND:
            diff = points - pb
            left = diff - diff // 2
            out[:, left:left + pb] = el
        else:   # Center: the first ceil(pb / 2) points stay, the last floor(pb / 2) move to the end
            right = pb // 2
            out[:, :pb - right] = el[:, :pb - right]
            out[:, points - right:] = el[:, pb - right:]
        self._put(out, self._rows)
        return 0

    def _rotate(self, forward):
        p = self.row_points()
        if p:
            shift = p - p // 2 if forward else p // 2   # out[i] = in[(i + shift) mod p]
            self._put(np.roll(self._el(), -shift, axis=1), self._rows)
        return self._ret()

    def swap_halves(self):
        return self._rotate(True)

    def fft_shift(self):
        return self._rotate(True)

    def ifft_shift(self):
        return self._rotate(False)

    def reverse(self):
        self._put(self._el()[:, ::-1], self._rows)
        return self._ret()

    def zero_interleave(self, factor):
        if factor <= 1:
            return self._ret()
        self._reserve(self.a.size * factor)
        out = np.zeros((self._rows, self.row_points(), factor, self._e()), self.dtype)
        out[:, :, 0, :] = self._el()
        self._put(out, self._rows)
        return self._ret()

    def decimatei(self, decimation_factor, delay):
        if decimation_factor == 0:
            return 7
        if self._rows:
            self._put(self._el()[:, delay::decimation_factor], self._rows)
        return self._ret()

    def mirror(self):
        if not self._complex and self._domain == TIME:
            return self._poison()
        assert self._complex, "the model covers half spectra held as complex rows"
        p = self.row_points()
        if self._rows and p:
            self._reserve(self._rows * 2 * (2 * p - 1))
            el = self._el()
            tail = el[:, :0:-1].copy()   # bins p - 1 .. 1, conjugated
            tail[:, :, 1] = _flip_sign(tail[:, :, 1])
            self._put(np.concatenate([el, tail], axis=1), self._rows)
        return self._ret()

    def conj(self):
        if not self._complex:
            return self._poison()
        el = self._el().copy()
        el[:, :, 1] = _flip_sign(el[:, :, 1])
        self._put(el, self._rows)
        return self._ret()

    def to_complex(self):
        if self._complex:
            return self._poison()
        self._reserve(2 * self.a.size)
        out = np.zeros((self._rows, self.row_len(), 2), self.dtype)
        out[:, :, 0] = self.a.reshape(self._rows, -1)
        self._complex = True
        self._put(out, self._rows)
        return self._ret()

    def _part(self, k):
        if not self._complex:
            return self._poison()
        part = self._el()[:, :, k]
        self._complex = False
        self._put(part, self._rows)
        return self._ret()

    def to_real(self):
        return self._part(0)

    def to_imag(self):
        return self._part(1)

    # ------------------------------------------------------------------ movers between matrices
    def _get_part(self, destinations, ks):
        if self.poisoned:
            return -1
        ok = self._complex and not any(d._complex for d in destinations)
        for d, k in zip(destinations, ks):
            if ok:
                d._reserve(max(self._rows * self.row_points(), 1))
                d._put(self._el()[:, :, k], self._rows)
            else:   # a real source or a complex destination: rows() empty rows
                d._put(np.zeros((self._rows, 0), self.dtype), self._rows)
        return 0

    def get_real(self, destination):
        return self._get_part([destination], [0])

    def get_imag(self, destination):
        return self._get_part([destination], [1])

    def get_real_imag(self, real, imag):
        return self._get_part([real, imag], [0, 1])

    def set_real_imag(self, real, imag):
        assert not real._complex and not imag._complex
        if real._rows != imag._rows or real.a.size != imag.a.size:
            return 7
        if self.poisoned:
            return -1
        self._reserve(max(2 * real.a.size, 1))
        self._complex = True
        self._put(np.stack([real.a, imag.a], axis=-1), real._rows)
        return 0

    # ------------------------------------------------------------------ rows in and out
    def get_row(self, row):
        if row >= self._rows:
            raise IndexError(row)
        return VecModel(self.a[row], self._complex, self._domain, self._delta)

    def set_row(self, row, vector):
        if row >= self._rows or vector.a.size != self.row_len():
            return 7
        self.a[row] = vector.a
        return self._ret()

    # ------------------------------------------------------------------ vector <-> matrix
    def _vec(self, a):
        return VecModel(a, self._complex, self._domain, self._delta)

    def to_interleaved(self):
        if self.poisoned:
            return -1, self._vec(np.zeros(0, self.dtype))
        return 0, self._vec(self._el().transpose(1, 0, 2).reshape(-1))

    @classmethod
    def from_interleaved(cls, vector, channels):
        if channels == 0 or vector.points() % channels:
            return 7, None
        e, p = 2 if vector._complex else 1, vector.points() // channels
        a = vector.a.reshape(p, channels, e).transpose(1, 0, 2).reshape(channels, p * e)
        return 0, cls(a, vector._complex, vector._domain, vector._delta)

    def overlap_add(self, hop):
        """y[r * hop : r * hop + F] += m[r] in ascending r from +0, in the matrix's dtype"""
        if hop == 0:
            return 7, None
        if self.poisoned:
            return -1, self._vec(np.zeros(0, self.dtype))
        rows, p, e = self._rows, self.row_points(), self._e()
        if rows == 0:
            return 0, self._vec(np.zeros(0, self.dtype))
        el = self._el()
        if hop >= p:   # no two rows meet: every position holds +0 + x or +0
            y = np.zeros((rows, hop, e), self.dtype)
            y[:, :p] += el
            y = y.reshape(-1)[:((rows - 1) * hop + p) * e]
        else:
            y = np.zeros(((rows - 1) * hop + p, e), self.dtype)
            for r in range(rows):
                y[r * hop:r * hop + p] += el[r]
        return 0, self._vec(y.reshape(-1))

    @classmethod
    def from_frames(cls, vector, frame_points, hop, pad_tail=False):
        if frame_points == 0 or hop == 0:
            return 7, None
        n, e = vector.points(), 2 if vector._complex else 1
        if pad_tail:
            rows = 0 if n == 0 else (1 if n <= frame_points else -((frame_points - n) // hop) + 1)
        else:
            rows = 0 if n < frame_points else (n - frame_points) // hop + 1
        idx = np.arange(rows)[:, None] * hop + np.arange(frame_points)[None, :]
        x = vector.a.reshape(n, e)
        out = np.zeros((rows, frame_points, e), vector.a.dtype)
        inside = idx < n
        out[inside] = x[idx[inside]]
        return 0, cls(out.reshape(rows, frame_points * e), vector._complex, vector._domain, vector._delta)

    @classmethod
    def from_vectors(cls, vectors, dtype=np.float32):
        vectors = list(vectors)
        if not vectors:
            return 0, cls(np.zeros((0, 0), dtype))
        v0 = vectors[0]
        if any(v.a.size != v0.a.size for v in vectors):
            return 7, None
        if any(v._complex != v0._complex or v._domain != v0._domain for v in vectors):
            return 2, None
        return 0, cls(np.stack([v.a for v in vectors]), v0._complex, v0._domain, v0._delta)


# ---------------------------------------------------------------------------------------------- one step, on either side
class ModelApi:
    """what apply_step needs of a side: the matrix class and a constructor from an array"""
    Mat = MatModel

    @staticmethod
    def mat(a, is_complex, domain, delta):
        return MatModel(a, is_complex, domain, delta)


# step kind -> the movers it runs
STEP_MOVERS = {k: (k,) for k in ("transpose", "zero_pad", "swap_halves", "fft_shift", "ifft_shift", "reverse",
                                 "zero_interleave", "decimatei", "mirror", "conj", "to_complex", "to_real", "to_imag",
                                 "get_real", "get_imag", "get_real_imag", "set_real_imag")}
STEP_MOVERS.update(row_move=("get_row", "set_row"), interleaved=("to_interleaved", "from_interleaved"),
                   frames=("overlap_add", "from_frames"), vectors=("get_row", "from_vectors"))


def apply_step(api, m, step):
    """Runs `step` = (kind, *args) on matrix m of either side (MatModel or DspMat: same methods, same codes).
    Returns (codes, the matrix the sequence goes on with, the other matrices and vectors the step read or wrote --
    all of them compared between the sides).  The steps between matrices give the other matrix another domain and
    delta than m's: a destination keeps its own."""
    kind, args = step[0], step[1:]
    dtype = m.dtype
    if kind in ("get_real", "get_imag"):
        dst = api.mat(np.ones((1, 1), dtype), False, 1 - m.domain(), 0.5)
        return [getattr(m, kind)(dst)], dst, [m]
    if kind == "get_real_imag":
        re = api.mat(np.ones((1, 1), dtype), False, 1 - m.domain(), 0.5)
        im = api.mat(np.ones((2, 3), dtype), False, m.domain(), 0.125)
        code = m.get_real_imag(re, im)
        return [code], (re, im)[args[0]], [m, (im, re)[args[0]]]
    if kind == "set_real_imag":   # m is the real part, the same rows in reverse order are the imaginary part
        im = api.mat(m.data()[::-1].copy(), False, m.domain(), m.delta())
        target = api.mat(np.ones((1, 2), dtype), True, 1 - m.domain(), 0.25)
        return [target.set_real_imag(m, im)], target, [m, im]
    if kind == "row_move":
        v = m.get_row(args[0])
        return [m.set_row(args[1], v)], m, [v]
    if kind == "interleaved":
        c1, v = m.to_interleaved()
        c2, out = api.Mat.from_interleaved(v, args[0])
        return [c1, c2], out, [m, v]
    if kind == "frames":   # hop = frame = the row's points: the matrix flattened and cut up again
        p = m.row_points()
        c1, v = m.overlap_add(p)
        c2, out = api.Mat.from_frames(v, p, p)
        return [c1, c2], out, [m, v]
    if kind == "vectors":
        vs = [m.get_row(r) for r in range(m.rows())]
        c, out = api.Mat.from_vectors(vs)
        return [c], out, [m, vs[0], vs[-1]]
    return [getattr(m, kind)(*args)], m, []


# ---------------------------------------------------------------------------------------------- the sequence generator
START_SHAPES = ((5, 1001), (3, 4096), (2, 4097), (257, 100), (1, 1), (7, 16))   # (rows, points)
SEEDS = tuple(range(24))


def _candidates(s, rng):
    """one (kind, *args) per mover step whose precondition holds in model state s and whose result keeps
    1 <= scalars <= MAX_SCALARS; the arguments are drawn here, the choice among the kinds by the caller"""
    rows, p, e, n = s.rows(), s.row_points(), s._e(), s.a.size
    cplx = s.is_complex()
    out = [("transpose",), ("swap_halves",), ("fft_shift",), ("ifft_shift",), ("reverse",)]
    max_p = MAX_SCALARS // (rows * e)
    if max_p > p:
        grow = (1, 2, 37, p // 2 + 1, p + 1, 3 * p)[rng.randint(6)]
        out.append(("zero_pad", min(p + grow, max_p), int(rng.randint(3))))
    f = int(rng.randint(2, 5))
    if n * f <= MAX_SCALARS:
        out.append(("zero_interleave", f))
    f = int(rng.randint(1, 6))
    out.append(("decimatei", f, int(rng.randint(0, min(p, f + 2)))))   # delay < points: at least one point stays
    if cplx:
        if rows * 2 * (2 * p - 1) <= MAX_SCALARS:
            out.append(("mirror",))
        out += [("conj",), ("to_real",), ("to_imag",), ("get_real",), ("get_imag",), ("get_real_imag", int(rng.randint(2)))]
    elif 2 * n <= MAX_SCALARS:
        out += [("to_complex",), ("set_real_imag",)]
    out.append(("row_move", int(rng.randint(rows)), int(rng.randint(rows))))
    total = rows * p
    ch = [c for c in (rows, p, 1, total, 2, 3, 5, 7, 16) if total % c == 0]
    out.append(("interleaved", ch[rng.randint(len(ch))]))
    out.append(("frames",))
    if rows <= 64:
        out.append(("vectors",))
    return out


def gen_sequence(rows, points, is_complex, seed, steps=STEPS):
    """The steps of one sequence and, per step, what happened: deterministic in its arguments; dtype and domain play
    no part (no mover looks at them, except mirror, which is drawn for complex rows only).  The last two steps are
    forced where the draw has not yet brought a transpose and a change of row_len."""
    rng = np.random.RandomState(seed * 1009 + rows * 31 + points * 7 + int(is_complex))
    e = 2 if is_complex else 1
    m = MatModel(np.zeros((rows, points * e), np.float32), is_complex)
    seq, log = [], []
    for i in range(steps):
        cand = _candidates(m, rng)
        step = cand[rng.randint(len(cand))]
        if i == steps - 2 and not any(ev["transpose"] for ev in log):
            step = ("transpose",)
        if i == steps - 1 and not any(ev["row_len_change"] for ev in log):
            forced = [c for c in cand if c[0] == "zero_pad"] or ([("decimatei", 2, 0)] if m.row_points() > 1 else []) or \
                [("transpose",)]
            step = forced[0]
        before = (m.a.size, m.row_len(), m.is_complex(), m.reallocs)
        codes, nxt, _ = apply_step(ModelApi, m, step)
        assert all(c == 0 for c in codes) and not nxt.poisoned and 1 <= nxt.a.size <= MAX_SCALARS, (step, codes)
        log.append(dict(step=step, movers=STEP_MOVERS[step[0]], transpose=step[0] == "transpose",
                        realloc=nxt.reallocs > (before[3] if nxt is m else 0),   # a new matrix starts at 0
                        shrink=nxt.a.size < before[0], space_change=nxt.is_complex() != before[2],
                        row_len_change=nxt.row_len() != before[1]))
        seq.append(step)
        m = nxt
    return seq, log


def all_sequences():
    """(rows, points, is_complex, seed) of every generated sequence: dtype and domain multiply them in the GPU test"""
    return [(r, p, c, s) for (r, p) in START_SHAPES for c in (False, True) for s in SEEDS]


def coverage(logs):
    """{mover: dict(count, after_transpose, after_realloc, after_shrink, after_space_change)} over the logs"""
    cov = {mv: dict(count=0, after_transpose=0, after_realloc=0, after_shrink=0, after_space_change=0) for mv in MOVERS}
    for log in logs:
        seen = dict(transpose=False, realloc=False, shrink=False, space_change=False)
        for ev in log:
            for mv in ev["movers"]:
                cov[mv]["count"] += 1
                for k in seen:
                    cov[mv]["after_" + k] += int(seen[k])
            for k in seen:
                seen[k] = seen[k] or ev[k]
    return cov


# ---------------------------------------------------------------------------------------------- dirty states
# Short fixed mover recipes that leave a matrix in a state a fresh one is never in.  (start rows, start points, steps);
# `None` for is_complex: both number spaces.
#
# D3: 3 x 1000 real scalars start with cap = 3000 + 3000 / 8 + 64 = 3439 = 19 * 181, which three equal rows cannot fill.
# zero_pad(1150) needs 3450 > 3439 and reallocates to 3450 + 3450 / 8 + 64 = 3450 + 431 + 64 = 3945 = 3 * 1315, so
# zero_pad(1315) then needs exactly 3945 == cap: no reallocation, and no scalar of slack behind the last row.
DIRTY = {
    "D1-shrunk": dict(shape=(5, 4097), is_complex=None, steps=[("decimatei", 4, 1)]),
    "D2-transposed": dict(shape=(1001, 5), is_complex=None, steps=[("transpose",)]),
    "D2-transposed-even": dict(shape=(1000, 5), is_complex=None, steps=[("transpose",)]),   # even N: for the sfft family's code 9
    "D3-exact-fit": dict(shape=(3, 1000), is_complex=False, steps=[("zero_pad", 1150, PAD_END), ("zero_pad", 1315, PAD_SURROUND)]),
    "D4-regrown": dict(shape=(3, 1000), is_complex=None, steps=[("zero_pad", 2000, PAD_CENTER), ("swap_halves",)]),
    "D5-space-twice": dict(shape=(5, 1001), is_complex=False, steps=[("to_complex",), ("to_real",)]),
    "D6-from-frames": dict(shape=None, is_complex=True, steps=[]),   # from_frames(4001 points, frame 64, hop 48, pad_tail)
    "D7-empty-rows": dict(shape=(5, 0), is_complex=None, steps=[]),
    "D7-no-rows": dict(shape=(0, 9), is_complex=None, steps=[]),
    "D7-empty-rows-transposed": dict(shape=(5, 0), is_complex=None, steps=[("transpose",)]),
    "D7-no-rows-transposed": dict(shape=(0, 9), is_complex=None, steps=[("transpose",)]),
}
D6_POINTS, D6_FRAME, D6_HOP = 4001, 64, 48


def build_dirty(api, name, fill, dtype, is_complex, domain, delta, vec=None):
    """The dirty state `name` on side `api`.  fill(rows, scalars per row) -> the start array; for D6 `vec(array)` makes
    the side's vector.  Returns the matrix."""
    d = DIRTY[name]
    if name == "D6-from-frames":
        code, m = api.Mat.from_frames(vec(fill(1, 2 * D6_POINTS).reshape(-1)), D6_FRAME, D6_HOP, True)
        assert code == 0
        return m
    rows, pts = d["shape"]
    m = api.mat(fill(rows, pts * (2 if is_complex else 1)), is_complex, domain, delta)
    for step in d["steps"]:
        codes, m, _ = apply_step(api, m, step)
        assert all(c == 0 for c in codes), (name, step, codes)
    return m
