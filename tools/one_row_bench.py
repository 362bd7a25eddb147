"""One long row through the row-aware kernels (second batch): this build against the parent commit's library on
one MI355X -> profiles/one_row_second_batch.txt.

  tools/build_baseline.sh <parent commit>      # -> tools/lab/old_lib/libbasic_dsp_hip_B.so
  python tools/one_row_bench.py --out profiles/one_row_second_batch.txt

The driver never touches the device.  It starts ONE child process at a time, each loading the library BDSP_HIP_LIBRARY
names, in the order parent, new, parent, new, ROUNDS rounds; every child has its own time limit, and the first child that
fails ends the run.  A child measures, per case, the median of SAMPLES samples of CALLS calls between two device events on
warmed buffers (one untimed sample first); a case leaves its vector with the length and delta it found (set_len after a
call that changes the length; the delayed resampling is timed as the pair up, down, which restores delta).  The children of
the first round also hash the result of one call of every case on fixed data, at the timed sizes and at SMALL points, real
and complex, f32 and f64.  Pair F, convolve(function) with 2 L + 1 > points, is a direct convolution of points^2 multiply-adds:
F_CALLS calls per sample up to F_MAX points, one call and F_SAMPLES_LONG samples up to F_MAX_LONG, not run above.

Per cell: median of the parent's round medians / of the new build's / margin = max - min of the parent's round medians.
A pair is slower when new > parent + margin at any size, in f32 or f64 (DESIGN 4.4's rule).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASELINE = os.path.join(ROOT, "tools", "lab", "old_lib", "libbasic_dsp_hip_B.so")
NEW = os.path.join(ROOT, "basic_dsp_amd", "lib", "libbasic_dsp_hip.so")
SIZES = (1 << 16, 1 << 20, 1 << 24)
SMALL = (1, 2, 3, 5, 85, 86, 128, 129, 255, 256, 257, 1000, 4097)
ROUNDS, SAMPLES, CALLS = 5, 5, 10
CHILD_LIMIT = 420  # seconds
F_MAX, F_CALLS, F_MAX_LONG, F_SAMPLES_LONG = 1 << 16, 2, 1 << 20, 2


def _ok(code):
    assert code == 0, code


def cases(bd, V, np, n, cplx, dtype, pairs=None):
    """(pair, name, make, call): make() -> a fresh object on fixed data; call(obj) runs the operation once and, unless
    call(obj, False), leaves obj with the shape and delta it had (None: prepare_argument_padded, hashed only)"""
    if pairs == "F":
        if n > F_MAX_LONG:
            return []
        tile = np.random.default_rng(n % 1000).uniform(-1.0, 1.0, min(n * (2 if cplx else 1), 1 << 20)).astype(dtype)
        host = np.resize(tile, n * (2 if cplx else 1))
        make = lambda: bd.DspVec(host, is_complex=cplx)  # noqa: E731
        out = [("F", "convolve sinc, L = points / 2 + 1", make, lambda v, restore=True: _ok(v.convolve(V.CONV_SINC, 0.25, n // 2 + 1))),
               ("F", "convolve raised_cosine, L = points", make, lambda v, restore=True: _ok(v.convolve(V.CONV_RAISED_COSINE, 0.25, n, 0.35)))]
        if cplx and n <= 4097:  # the host samples the callback 2 L + 1 times
            out.append(("F", "convolve_complex, L = points", make,
                        lambda v, restore=True: _ok(v.convolve_complex(lambda t: complex(0.5 - 0.01 * t, 0.02 * t), 0.25, n))))
        return out
    e = 2 if cplx else 1
    sfx = "32" if dtype == np.float32 else "64"
    rng = np.random.default_rng(n % 1000 + 7 * e)
    tile = rng.uniform(-1.0, 1.0, min(n * e, 1 << 20)).astype(dtype)
    host = np.resize(tile, n * e)
    set_len = getattr(bd.lib, "set_len" + sfx)

    def vec(domain=V.TIME):
        return lambda: bd.DspVec(host, is_complex=cplx, domain=domain)

    def keep(fn):
        def call(v, restore=True):
            assert fn(v) == 0
            if restore:
                set_len(v._h, n * e)
        return call

    out = []
    for w, wn in enumerate(("triangular", "hamming", "blackman_harris", "rectangular", "hann")):
        out.append(("A", "apply_window " + wn, vec(), keep(lambda v, w=w: v.apply_window(w))))
        out.append(("A", "unapply_window " + wn, vec(), keep(lambda v, w=w: v.unapply_window(w))))
    for f, fn in ((V.CONV_SINC, "sinc"), (V.CONV_RAISED_COSINE, "raised_cosine")):
        out.append(("B", "multiply_frequency_response " + fn, vec(V.FREQ),
                    keep(lambda v, f=f: v.multiply_frequency_response(f, 0.5, 0.35))))
    for f in (2, 3):
        out.append(("C", "interpolatei sinc x%d" % f, vec(), keep(lambda v, f=f: v.interpolatei(V.CONV_SINC, f))))
    out.append(("C", "interpolatei raised_cosine x2", vec(), keep(lambda v: v.interpolatei(V.CONV_RAISED_COSINE, 2, 0.35))))
    up, down = n + n // 2, max(n - n // 4, 1)
    out.append(("C", "interpolate sinc up", vec(), keep(lambda v: v.interpolate(V.CONV_SINC, up))))
    out.append(("C", "interpft up", vec(), keep(lambda v: v.interpft(up))))
    if down < n:
        out.append(("C", "interpolate sinc down", vec(), keep(lambda v: v.interpolate(V.CONV_SINC, down))))

        def up_down(v, restore=True):  # 2 n and back: delta is restored exactly
            assert v.interpolate(V.CONV_RAISED_COSINE, 2 * n, 0.3, 0.35) == 0
            assert v.interpolate(V.CONV_SINC, n, 0.3) == 0
        out.append(("C", "interpolate delayed up, down", vec(), up_down))
    out.append(("H", "interpolate equal length, delayed", vec(), keep(lambda v: v.interpolate(V.CONV_SINC, n, 0.3))))
    out.append(("D", "decimatei 2, 1", vec(), keep(lambda v: v.decimatei(2, 1))))
    out.append(("D", "decimatei 3, 0", vec(), keep(lambda v: v.decimatei(3, 0))))
    if not cplx:
        out.append(("E", "interpolate_lin 1.5, 0.25", vec(), keep(lambda v: v.interpolate_lin(1.5, 0.25))))
        out.append(("E", "interpolate_hermite 1.5, 0.25", vec(), keep(lambda v: v.interpolate_hermite(1.5, 0.25))))
        out.append(("E", "interpolate_hermite 0.75, 0", vec(), keep(lambda v: v.interpolate_hermite(0.75, 0.0))))
    # G: rows Surround-padded to l points by correlate's general path (l above the fused kernel's 4096) and by
    # prepare_argument_padded; decimatei(2, 0) brings the rows back from l = 2 p to p
    if n >= 8192:
        for rows in (1, n // 8192) if n > 8192 else (1,):
            p = n // rows // 2
            if cplx:
                arg = bd.DspVec(np.resize(tile, 4 * p), is_complex=True, domain=V.FREQ)

                def corr(m, restore=True, arg=arg):
                    assert m.correlate(arg) == 0 and (not restore or m.decimatei(2, 0) == 0)
                out.append(("G", "mat correlate %s rows, decimatei" % ("1" if rows == 1 else "n / 8192"),
                            lambda rows=rows, p=p: bd.DspMat(np.resize(tile, rows * 2 * p).reshape(rows, 2 * p), is_complex=True), corr))
    if n > 1:
        rows = 1 if n < 4096 else 16
        out.append(("G", "mat prepare_argument_padded (bits only)",
                    lambda: bd.DspMat(np.resize(tile, rows * (n // rows) * e).reshape(rows, (n // rows) * e), is_complex=cplx), None))
    return out


def child(sizes, bits, pairs):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import numpy as np
    import basic_dsp_amd as bd
    from basic_dsp_amd import vector as V
    bd.require_gpu()
    L = bd.lib
    ev0, ev1 = L.bdsp_hip_event_create(), L.bdsp_hip_event_create()
    ms = C.c_float()

    def sample(call, obj, calls):
        assert L.bdsp_hip_event_record(ev0, None) == 0
        for _ in range(calls):
            call(obj)
        assert L.bdsp_hip_event_record(ev1, None) == 0
        assert L.bdsp_hip_synchronize(None) == 0
        assert L.bdsp_hip_event_elapsed_ms(ev0, ev1, C.byref(ms)) == 0
        return ms.value * 1e3 / calls

    res = {"lib": bd.LIB_PATH, "us": {}, "sha": {}}
    combos = [(c, d) for d in (np.float32, np.float64) for c in (True, False)]
    for n in (list(SMALL) if bits else []) + list(sizes):
        for cplx, dtype in combos:
            timed = n in sizes and (cplx, dtype) in ((True, np.float32), (False, np.float64))
            tag = "%s %s" % ("complex" if cplx else "real", np.dtype(dtype).name)
            for pair, name, make, call in cases(bd, V, np, n, cplx, dtype, pairs):
                key = "%s|%s|%d|%s" % (pair, name, n, tag)
                if bits:
                    obj = make()
                    if call is None:
                        assert obj.prepare_argument_padded() == 0
                    else:
                        call(obj, False)
                    res["sha"][key] = hashlib.sha1(np.ascontiguousarray(obj.data()).tobytes()).hexdigest()
                    del obj
                # complex f32 and real f64; interpolate_lin needs real data and correlate complex: those in both precisions
                if call is not None and n in sizes and (timed or pair == "E" or (pair == "G" and cplx)):
                    calls, samples = CALLS, SAMPLES
                    if pair == "F":
                        if "convolve_complex" in name:
                            continue
                        calls, samples = (F_CALLS, SAMPLES) if n <= F_MAX else (1, F_SAMPLES_LONG)
                    obj = make()
                    sample(call, obj, calls)
                    res["us"][key] = float(np.median([sample(call, obj, calls) for _ in range(samples)]))
                    del obj
    print("ONE_ROW " + json.dumps(res), flush=True)


def run_child(lib, sizes, bits, pairs, log):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--sizes", ",".join(str(s) for s in sizes)] + (["--bits"] if bits else [])
    cmd += ["--pairs", pairs] if pairs else []
    try:
        r = subprocess.run(cmd, env=dict(os.environ, BDSP_HIP_LIBRARY=lib), capture_output=True, text=True, timeout=CHILD_LIMIT, cwd=ROOT)
    except subprocess.TimeoutExpired:
        log("FAILED: a child passed its limit of %d s: nothing more is started" % CHILD_LIMIT)
        sys.exit(1)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ONE_ROW ")]
    if r.returncode != 0 or not lines:
        log("FAILED (%d): nothing more is started\n%s" % (r.returncode, (r.stdout + r.stderr)[-3000:]))
        sys.exit(1)
    return json.loads(lines[-1][8:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--bits", action="store_true")
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--pairs", choices=("F",), help="F: pair F alone, against a build whose vector takes mt_conv_direct")
    ap.add_argument("--parent-lib", default=BASELINE)
    ap.add_argument("--new-lib", default=NEW)
    ap.add_argument("--out")
    a = ap.parse_args()
    sizes = tuple(int(s) for s in a.sizes.split(","))
    if a.child:
        return child(sizes, a.bits, a.pairs)
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    import numpy as np
    log("# tools/one_row_bench.py: one long row, the parent commit's library against this build, on one MI355X.")
    log("# order parent, new, %d rounds, one fresh process each; per round the median of %d samples of %d calls between device" % (a.rounds, SAMPLES, CALLS))
    log("# events on warmed buffers; us per call.  margin = max - min of the parent's round medians; slower: new > parent + margin.")
    runs = {"parent": [], "new": []}
    for rnd in range(a.rounds):
        for who, lib in (("parent", a.parent_lib), ("new", a.new_lib)):
            runs[who].append(run_child(lib, sizes, rnd == 0, a.pairs, log))
            log("# round %d %s: %d timed cases" % (rnd + 1, who, len(runs[who][-1]["us"])))
    sha_p, sha_n = runs["parent"][0]["sha"], runs["new"][0]["sha"]
    assert sha_p.keys() == sha_n.keys()
    differ = sorted(k for k in sha_p if sha_p[k] != sha_n[k])
    log("# results hashed: %d (operations x options x points x number space x precision); byte-identical: %d" % (len(sha_p), len(sha_p) - len(differ)))
    for k in differ:
        log("DIFFERENT BITS  " + k)
    log("%-4s %-42s %9s %-14s %28s" % ("pair", "operation", "points", "data", "parent / new / margin (us)"))
    verdict = {}
    for key in runs["parent"][0]["us"]:
        pair, name, n, tag = key.split("|")
        p = [r["us"][key] for r in runs["parent"]]
        q = [r["us"][key] for r in runs["new"]]
        mp, mq, margin = float(np.median(p)), float(np.median(q)), max(p) - min(p)
        slow = mq > mp + margin
        verdict.setdefault(pair, []).append(slow)
        log("%-4s %-42s %9s %-14s %9.1f / %9.1f / %6.1f%s" % (pair, name, "2^%d" % (int(n).bit_length() - 1), tag, mp, mq, margin, "  SLOWER" if slow else ""))
    for pair in sorted(verdict):
        bad = sorted(k for k in differ if k.startswith(pair + "|"))
        log("# pair %s: %d of %d cells slower, %d results differ -> %s" % (pair, sum(verdict[pair]), len(verdict[pair]), len(bad),
                                                                        "stays as the parent has it" if (any(verdict[pair]) or bad) else "unified"))


if __name__ == "__main__":
    main()
