"""A numpy model of DspVec's "movers" -- the operations whose result is a bit-exact rearrangement of their input
(copies, zeros, sign-bit flips) -- written from basic_dsp_amd/vector.py and the facade's contract as index arithmetic
only: it never calls the library.  Every mover is one gather: out[i] = in[idx[i]] (idx < 0: +0.0), with the sign bit
flipped where `flip` says so.  VecModel answers the same methods with the same codes, metadata changes and poisoning as
DspVec, so one driver (apply_step) runs a step on either side; tests/test_vec_model.py pins every mover against
oracle_lib and tests/test_gpu_vec_sequences.py runs generated mover sequences on the GPU against the model.

Three things a fresh vector never shows are kept next to the data:
  * cap: the allocation's capacity by the library's rule (a buffer that is too small grows to n + n / 8 + 64 scalars,
    never shrinks, clone() starts over from the valid length) -- compared with allocated_len() at every GPU step;
  * trades: how often the live buffer and the trade buffer changed places (odd: `data` is what was `buf`);
  * unspec: set_len() can grow a vector within its allocation, and what the grown tail holds is not specified.  Those
    scalars are marked, the mark moves with the scalar through every later mover (a zero written over it clears it), and
    the comparison skips exactly the marked scalars.
"""
import numpy as np

TIME, FREQ = 0, 1
PAD_END, PAD_SURROUND, PAD_CENTER = 0, 1, 2
MAX_SCALARS = 1 << 20
STEPS = 16

MOVERS = ("swap_halves", "fft_shift", "ifft_shift", "reverse", "zero_pad", "zero_interleave", "decimatei", "mirror", "conj",
          "to_complex", "to_real", "to_imag", "get_real", "get_imag", "get_real_imag", "set_real_imag", "split_into", "merge",
          "clone", "set_len")
# read at every step of the GPU sequences (device_ptr is an address: the model has none)
ACCESSORS = ("len", "points", "is_complex", "domain", "delta", "allocated_len", "data", "datac", "device_ptr", "is_erroneous")
# plumbing of the wrapper, exercised by every test that builds a vector or edits one scalar
PLUMBING = ("overwrite_data", "set_value")


def grown_cap(n):
    """what a buffer that must hold n scalars and is too small grows to"""
    return n + n // 8 + 64


class VecModel:
    def __init__(self, a, is_complex=False, domain=TIME, delta=1.0):
        a = np.array(a, copy=True).reshape(-1)
        assert a.dtype in (np.float32, np.float64)
        assert not (is_complex and a.size % 2), "a complex vector has an even scalar length"
        self.dtype = a.dtype.type
        self.a = a
        self.unspec = np.zeros(a.size, bool)
        self._complex, self._domain = bool(is_complex), int(domain)
        self._delta = float(self.dtype(delta))
        self.cap = grown_cap(max(a.size, 1))
        self.reallocs = 0   # reallocations by calls, after the constructor's allocation
        self.trades = 0

    # ------------------------------------------------------------------ metadata, as DspVec
    def __len__(self):
        return self.a.size

    def len(self):
        return self.a.size

    def points(self):
        return self.a.size // self._e()

    def is_complex(self):
        return self._complex

    def domain(self):
        return self._domain

    def delta(self):
        return self._delta

    def allocated_len(self):
        return self.cap

    def is_erroneous(self):
        return self.a.size == 0 and np.isnan(self._delta)

    def data(self):
        return self.a.copy()

    # ------------------------------------------------------------------ helpers
    def _e(self):
        return 2 if self._complex else 1

    def _reserve(self, n):
        if n > self.cap:
            self.cap = grown_cap(n)
            self.reallocs += 1

    def _ret(self, code=0):
        """the facade's rule: an error code as it is, else -1 for a poisoned vector, else 0"""
        return -1 if code == 0 and self.is_erroneous() else code

    def _poison(self):
        self.a, self.unspec = np.zeros(0, self.dtype), np.zeros(0, bool)
        self._delta = float("nan")
        return -1

    def _gather(self, idx, flip=None, trade=True):
        """out[i] = a[idx[i]], +0.0 where idx[i] < 0, sign bit flipped where flip[i]"""
        idx = np.asarray(idx, np.int64).reshape(-1)
        src = np.concatenate([self.a, np.zeros(1, self.dtype)])      # idx -1 reads the zero at the end
        out = src[idx]
        if flip is not None:
            u = out.view(np.uint32 if self.dtype == np.float32 else np.uint64)
            u[np.asarray(flip, bool).reshape(-1)] ^= u.dtype.type(1) << u.dtype.type(8 * out.itemsize - 1)
        self.unspec = np.concatenate([self.unspec, np.zeros(1, bool)])[idx]
        self.a = out
        self.trades += int(trade)

    def _point_idx(self, point_idx):
        """scalar indices of the points point_idx (-1 stays -1)"""
        point_idx = np.asarray(point_idx, np.int64)
        e = self._e()
        s = point_idx[:, None] * e + np.arange(e)[None, :]
        s[point_idx < 0] = -1
        return s.reshape(-1)

    # ------------------------------------------------------------------ movers, in place
    def _rotate(self, forward):
        p = self.points()
        if p:
            shift = p - p // 2 if forward else p // 2   # out[i] = in[(i + shift) mod p]
            self._gather(self._point_idx((np.arange(p) + shift) % p))
        return self._ret()

    def swap_halves(self):
        return self._rotate(True)

    def fft_shift(self):
        return self._rotate(True)

    def ifft_shift(self):
        return self._rotate(False)

    def reverse(self):
        p = self.points()
        if p:
            self._gather(self._point_idx(np.arange(p)[::-1]))
        return self._ret()

    def zero_pad(self, points, option=PAD_END):
        e, pb = self._e(), self.points()
        if points * e <= self.a.size:
            return 7   # an argument error comes first, poisoned or not
        self._reserve(points * e)
        idx = np.full(points, -1, np.int64)
        if option == PAD_END:
            idx[:pb] = np.arange(pb)
        elif option == PAD_SURROUND:
            diff = points - pb
            left = diff - diff // 2
            idx[left:left + pb] = np.arange(pb)
        else:   # Center: the first ceil(pb / 2) points stay, the last floor(pb / 2) move to the end
            right = pb // 2
            idx[:pb - right] = np.arange(pb - right)
            idx[points - right:] = np.arange(pb - right, pb)
        self._gather(self._point_idx(idx))
        return self._ret()   # (a poisoned vector that was padded holds zeros and a NaN delta: no longer "erroneous")

    def zero_interleave(self, factor):
        if factor <= 1:
            return self._ret()
        p = self.points()
        self._reserve(self.a.size * factor)
        idx = np.full((p, factor), -1, np.int64)
        idx[:, 0] = np.arange(p)
        self._gather(self._point_idx(idx.reshape(-1)))
        return self._ret()

    def decimatei(self, decimation_factor, delay):
        if decimation_factor == 0:
            return 7
        keep = np.arange(self.points())[delay::decimation_factor]
        if keep.size:
            self._gather(self._point_idx(keep))
        else:   # no launch, no trade
            self.a, self.unspec = np.zeros(0, self.dtype), np.zeros(0, bool)
        return self._ret()

    def mirror(self):
        if not self._complex and self._domain == TIME:
            return self._poison()
        assert self._complex, "the model covers half spectra held as complex vectors"
        p = self.points()
        if p:
            self._reserve(2 * (2 * p - 1))
            pts = np.concatenate([np.arange(p), np.arange(p - 1, 0, -1)])   # bins 0 .. p - 1, then p - 1 .. 1 conjugated
            flip = np.zeros((2 * p - 1, 2), bool)
            flip[p:, 1] = True
            self._gather(self._point_idx(pts), flip)
        return self._ret()

    def conj(self):
        if not self._complex:
            return self._poison()
        flip = np.zeros((self.points(), 2), bool)
        flip[:, 1] = True
        self._gather(np.arange(self.a.size), flip, trade=False)   # in place
        return self._ret()

    def to_complex(self):
        if self._complex:
            return self._poison()
        n = self.a.size
        self._reserve(2 * n)
        idx = np.full((n, 2), -1, np.int64)
        idx[:, 0] = np.arange(n)
        self._gather(idx.reshape(-1))
        self._complex = True
        return self._ret()

    def _part(self, k):
        if not self._complex:
            return self._poison()
        self._gather(2 * np.arange(self.points()) + k)
        self._complex = False
        return self._ret()

    def to_real(self):
        return self._part(0)

    def to_imag(self):
        return self._part(1)

    def set_len(self, n):
        """the C ABI's set_len: ignored for an odd length of a complex vector; grows within (or past) the allocation, and
        what the grown tail holds is not specified"""
        if self._complex and n % 2:
            return
        self._reserve(n)
        old = self.a.size
        keep = min(old, n)
        self.a = np.concatenate([self.a[:keep], np.zeros(n - keep, self.dtype)])
        self.unspec = np.concatenate([self.unspec[:keep], np.ones(n - keep, bool)])

    def clone(self):
        c = VecModel(self.a, self._complex, self._domain, 1.0)
        c._delta = self._delta
        c.unspec = self.unspec.copy()
        return c

    # ------------------------------------------------------------------ movers between vectors
    def _write(self, a, unspec):
        """another vector's call wrote this one's live buffer: resized, no trade, own domain / delta / number space"""
        self._reserve(max(a.size, 1))
        self.a, self.unspec = np.array(a, self.dtype), np.array(unspec, bool)

    def _get_part(self, destinations, ks):
        """the getters run on a clone that the facade consumes and answer 9 (the facade's convert_void), whatever
        happened: a real source or a complex destination empties every destination"""
        ok = self._complex and not any(d._complex for d in destinations)
        for d, k in zip(destinations, ks):
            if ok:
                d._write(self.a[k::2], self.unspec[k::2])
            else:
                d.a, d.unspec = np.zeros(0, d.dtype), np.zeros(0, bool)
        return 9

    def get_real(self, destination):
        return self._get_part([destination], [0])

    def get_imag(self, destination):
        return self._get_part([destination], [1])

    def get_real_imag(self, real, imag):
        return self._get_part([real, imag], [0, 1])

    def set_real_imag(self, real, imag):
        assert self._complex and not real._complex and not imag._complex, "the model covers complex targets of real parts"
        if real.a.size != imag.a.size:
            return 7
        self._write(np.stack([real.a, imag.a], axis=-1).reshape(-1), np.stack([real.unspec, imag.unspec], axis=-1).reshape(-1))
        return self._ret()

    def split_into(self, targets):
        """point i goes to target i % n, position i / n; 9 on success (convert_void)"""
        n = len(targets)
        if n == 0 or self.a.size % n:
            return 7
        tlen = self.a.size // n
        assert all(t._complex == self._complex for t in targets), "the model covers targets of the source's number space"
        if self._complex and tlen % 2:
            return 13
        e = self._e()
        for k, t in enumerate(targets):
            t._write(self.a.reshape(-1, n, e)[:, k].reshape(-1), self.unspec.reshape(-1, n, e)[:, k].reshape(-1))
        return 9

    def merge(self, sources):
        n = len(sources)
        if n == 0 or any(s.a.size != sources[0].a.size for s in sources):
            return 7
        assert all(s._complex == self._complex for s in sources), "the model covers sources of the target's number space"
        e = self._e()
        self._write(np.stack([s.a.reshape(-1, e) for s in sources], axis=1).reshape(-1),
                    np.stack([s.unspec.reshape(-1, e) for s in sources], axis=1).reshape(-1))
        return self._ret()


# ---------------------------------------------------------------------------------------------- one step, on either side
class ModelApi:
    """what apply_step needs of a side: a constructor from an array, and set_len (DspVec has no wrapper for it)"""

    @staticmethod
    def vec(a, is_complex, domain, delta):
        return VecModel(a, is_complex, domain, delta)

    @staticmethod
    def set_len(v, n):
        v.set_len(n)


def _small(api, v, scalars, cplx, delta):
    """a destination of `scalars` ones with another domain and delta than v's: a destination keeps its own"""
    return api.vec(np.ones(scalars, v.dtype), cplx, 1 - v.domain(), delta)


def apply_step(api, v, step):
    """Runs `step` = (kind, *args) on vector v of either side (VecModel or DspVec: same methods, same codes).  Returns
    (codes, the vector the sequence goes on with, the other vectors the step read or wrote -- all compared between the
    sides)."""
    kind, args = step[0], step[1:]
    if kind == "set_len":
        api.set_len(v, args[0])
        return [], v, []
    if kind in ("get_real", "get_imag"):
        dst = _small(api, v, 5, False, 0.5)
        return [getattr(v, kind)(dst)], dst, [v]
    if kind == "get_real_imag":
        re, im = _small(api, v, 5, False, 0.5), _small(api, v, 3, False, 0.125)
        code = v.get_real_imag(re, im)
        return [code], (re, im)[args[0]], [v, (im, re)[args[0]]]
    if kind == "set_real_imag":   # v is the real part, its reverse (made on the same side) the imaginary part
        im = v.clone()
        c1 = im.reverse()
        target = _small(api, v, 2, True, 0.25)
        return [c1, target.set_real_imag(v, im)], target, [v, im]
    if kind == "split_merge":     # n targets of 5 (real) / 4 (complex) scalars, merged again in reverse order
        n = args[0]
        targets = [_small(api, v, 4 if v.is_complex() else 5, v.is_complex(), 0.5) for _ in range(n)]
        c1 = v.split_into(targets)
        out = _small(api, v, 2, v.is_complex(), 0.25)
        c2 = out.merge(targets[::-1])
        return [c1, c2], out, [v] + targets
    if kind == "clone":
        return [], v.clone(), [v]
    return [getattr(v, kind)(*args)], v, []


STEP_MOVERS = {k: (k,) for k in MOVERS if k not in ("split_into", "merge")}
STEP_MOVERS["split_merge"] = ("split_into", "merge")
STEP_MOVERS["set_real_imag"] = ("clone", "reverse", "set_real_imag")

# ---------------------------------------------------------------------------------------------- the sequence generator
START_POINTS = (1, 16, 1001, 4096, 4097, 25700)
SEEDS = tuple(range(16))
EXACT_FIT_AT = (4, 10)   # the steps at which the generator makes len == cap where the state allows it


def _candidates(s, rng):
    """one (kind, *args) per mover step whose precondition holds in model state s and whose result keeps
    1 <= scalars <= MAX_SCALARS; the arguments are drawn here, the choice among the kinds by the caller"""
    p, e, n, cplx = s.points(), s._e(), s.a.size, s.is_complex()
    out = [("swap_halves",), ("fft_shift",), ("ifft_shift",), ("reverse",), ("clone",)]
    max_p = MAX_SCALARS // e
    if max_p > p:
        grow = (1, 2, 37, p // 2 + 1, p + 1, 3 * p)[rng.randint(6)]
        out.append(("zero_pad", min(p + grow, max_p), int(rng.randint(3))))
    f = int(rng.randint(2, 5))
    if n * f <= MAX_SCALARS:
        out.append(("zero_interleave", f))
    f = int(rng.randint(1, 6))
    out.append(("decimatei", f, int(rng.randint(0, min(p, f + 2)))))   # delay < points: at least one point stays
    # set_len: shorter, or longer within the allocation, or past it
    choices = [max(e, (n // 2) // e * e), max(e, n - e), min(n + 3 * e, MAX_SCALARS), min((s.cap + 7 * e) // e * e, MAX_SCALARS)]
    out.append(("set_len", int(choices[rng.randint(len(choices))])))
    if cplx:
        if 2 * (2 * p - 1) <= MAX_SCALARS:
            out.append(("mirror",))
        out += [("conj",), ("to_real",), ("to_imag",), ("get_real",), ("get_imag",), ("get_real_imag", int(rng.randint(2)))]
    elif 2 * n <= MAX_SCALARS:
        out += [("to_complex",), ("set_real_imag",)]
    div = [d for d in (1, 2, 3, 4, 5, 7) if p % d == 0]
    out.append(("split_merge", div[rng.randint(len(div))]))
    return out


def _exact_fit_step(s, rng):
    """a step that makes len == cap without a reallocation, or None where none exists (len == cap already, or a complex
    vector in an allocation of odd capacity)"""
    e, n = s._e(), s.a.size
    if n >= s.cap or s.cap % e or s.cap > MAX_SCALARS:
        return None
    return ("zero_pad", s.cap // e, int(rng.randint(3))) if rng.randint(3) else ("set_len", s.cap)


def gen_sequence(points, is_complex, seed, steps=STEPS):
    """The steps of one sequence and, per step, the state it started from and what it did: deterministic in its
    arguments; dtype and domain play no part (no mover looks at them, except mirror, which is drawn for complex vectors
    only)."""
    rng = np.random.RandomState(seed * 1009 + points * 7 + int(is_complex))
    v = VecModel(np.zeros(points * (2 if is_complex else 1), np.float32), is_complex)
    seq, log = [], []
    for i in range(steps):
        cand = _candidates(v, rng)
        step = cand[rng.randint(len(cand))]
        if i in EXACT_FIT_AT:
            step = _exact_fit_step(v, rng) or step
        before = dict(n=v.a.size, cplx=v.is_complex(), reallocs=v.reallocs, odd_trades=v.trades % 2 == 1, exact_fit=v.a.size == v.cap)
        codes, nxt, _ = apply_step(ModelApi, v, step)
        assert all(c in (0, 9) for c in codes) and not nxt.is_erroneous() and 1 <= nxt.a.size <= MAX_SCALARS, (step, codes)
        log.append(dict(step=step, movers=STEP_MOVERS[step[0]], odd_trades=before["odd_trades"], exact_fit=before["exact_fit"],
                        realloc=nxt.reallocs > (before["reallocs"] if nxt is v else 0),   # a new vector starts at 0
                        shrink=nxt.a.size < before["n"], space_change=nxt.is_complex() != before["cplx"]))
        seq.append(step)
        v = nxt
    return seq, log


def all_sequences():
    """(points, is_complex, seed) of every generated sequence: dtype and domain multiply them in the GPU test"""
    return [(p, c, s) for p in START_POINTS for c in (False, True) for s in SEEDS]


HISTORIES = ("after_realloc", "after_shrink", "after_space_change", "odd_trades", "exact_fit")


def coverage(logs):
    """{mover: count and, per history, how often the mover ran with it}: after_* -- the event happened at an earlier step
    of the sequence; odd_trades / exact_fit -- the state the step started from (buffers in swapped places; len == cap)"""
    cov = {mv: dict(count=0, **{h: 0 for h in HISTORIES}) for mv in MOVERS}
    for log in logs:
        seen = dict(realloc=False, shrink=False, space_change=False)
        for ev in log:
            for mv in ev["movers"]:
                cov[mv]["count"] += 1
                for k in seen:
                    cov[mv]["after_" + k] += int(seen[k])
                cov[mv]["odd_trades"] += int(ev["odd_trades"])
                cov[mv]["exact_fit"] += int(ev["exact_fit"])
            for k in seen:
                seen[k] = seen[k] or ev[k]
    return cov


# ---------------------------------------------------------------------------------------------- dirty states
# Short fixed mover recipes that leave a vector in a state a fresh one is never in: (start points, number space(s), steps).
# `None` for is_complex: both number spaces.  "-even" / "-odd": the length the recipe ends with, for the FFT family.
#
# exact fit, real: 3000 scalars start with cap = 3000 + 375 + 64 = 3439; zero_pad(3439) needs exactly the allocation.
# exact fit, complex: 1504 points = 3008 scalars start with cap = 3008 + 376 + 64 = 3448 = 2 * 1724.
DIRTY = {
    "shrunk-even": dict(points=4097, is_complex=None, steps=[("decimatei", 4, 1)]),           # 1024 points: (4097 - 1 + 3) // 4
    "shrunk-odd": dict(points=4097, is_complex=None, steps=[("decimatei", 4, 1), ("decimatei", 1, 1)]),   # 1023 points
    "shrunk-by-set_len": dict(points=2001, is_complex=None, steps=[("set_len", 2000)]),
    "shrunk-by-set_len-odd": dict(points=2001, is_complex=False, steps=[("set_len", 1001)]),
    "odd-trades": dict(points=1000, is_complex=None, steps=[("swap_halves",)]),
    "odd-trades-odd": dict(points=1001, is_complex=None, steps=[("swap_halves",)]),
    "exact-fit-real": dict(points=3000, is_complex=False, steps=[("zero_pad", 3439, PAD_END)]),
    "exact-fit-complex": dict(points=1504, is_complex=True, steps=[("zero_pad", 1724, PAD_END)]),
    "regrown": dict(points=1000, is_complex=None, steps=[("zero_pad", 2000, PAD_CENTER), ("swap_halves",)]),
    "regrown-odd": dict(points=1000, is_complex=None, steps=[("zero_pad", 2001, PAD_CENTER), ("swap_halves",)]),
    "space-twice": dict(points=1001, is_complex=False, steps=[("to_complex",), ("to_real",)]),
    "get_real-destination": dict(points=1001, is_complex=True, steps=[("get_real",)]),
    "split_into-target": dict(points=2002, is_complex=None, steps=[("split_target", 2)]),
    "clone-of-dirty": dict(points=1000, is_complex=None, steps=[("zero_pad", 2001, PAD_CENTER), ("swap_halves",), ("clone",)]),
    "emptied-and-refilled": dict(points=1001, is_complex=None, steps=[("refill",)]),
    "empty": dict(points=0, is_complex=None, steps=[]),
}


def build_dirty(api, name, fill, is_complex, domain, delta):
    """The dirty state `name` on side `api`.  fill(scalars, k) -> the k-th start array.  Returns the vector; its
    number space is the recipe's result (get_real-destination and space-twice end real)."""
    d = DIRTY[name]
    e = 2 if is_complex else 1
    v = api.vec(fill(d["points"] * e, 0), is_complex, domain, delta)
    for step in d["steps"]:
        if step[0] == "split_target":     # the first of n targets, which started as 5 / 4 scalars
            targets = [api.vec(np.ones(4 if is_complex else 5, v.dtype), is_complex, domain, delta) for _ in range(step[1])]
            assert v.split_into(targets) == 9
            v = targets[0]
        elif step[0] == "refill":         # decimatei with delay >= points empties the vector; merge of two fills it again
            assert v.decimatei(3, v.points()) == 0 and v.len() == 0
            parts = [api.vec(fill(500 * e, 1 + k), is_complex, domain, delta) for k in range(2)]
            assert v.merge(parts) == 0
        elif step[0] == "get_real":       # the destination goes on: it keeps the domain and delta it was made with
            dst = api.vec(np.ones(5, v.dtype), False, domain, delta)
            assert v.get_real(dst) == 9
            v = dst
        else:
            codes, v, _ = apply_step(api, v, step)
            assert all(c == 0 for c in codes), (name, step, codes)
    return v
