"""CPU-only checks of the launch helper (kernel_lds / kernel_slots: bdsp_internal.h, runtime.cpp, launch_cache_core.h):
the cache behind it holds under eight threads and keeps the devices apart (tests/host_sim/sim_launch_cache.cpp, a
stand-alone program built plainly and with the thread sanitizer), the two runtime calls it wraps occur nowhere else in the
library's sources, no launcher keeps a function-level static, the register-resident transforms' descriptor is defined
once, and the Makefile's HDRS names every header the units include."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_dsp_amd", "csrc")


def sources():
    return {n: open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith((".h", ".hip", ".cpp"))}


def test_the_cache_under_8_threads_and_3_devices(tmp_path):
    """8 threads x 1000 lookups over 3 device ordinals x 4 (kernel, threads, lds) keys: the query runs exactly 12 times,
    every lookup returns its own device's value, a result below 1 comes back as 1; plainly and under -fsanitize=thread."""
    src = os.path.join(ROOT, "tests", "host_sim", "sim_launch_cache.cpp")
    text = open(src).read()
    assert re.search(r"^int main\(\)", text, re.M) and '#include "../../basic_dsp_amd/csrc/launch_cache_core.h"' in text
    assert "THREADS = 8, LOOKUPS = 1000, DEVICES = 3, KEYS = 4" in text
    for flags, name in (([], "sim_launch_cache"), (["-fsanitize=thread", "-g"], "sim_launch_cache_tsan")):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread"] + flags + ["-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (name, r.stdout[-3000:], r.stderr[-3000:])
        assert "FAIL" not in r.stdout and "ThreadSanitizer" not in r.stderr, (name, r.stdout[-3000:], r.stderr[-3000:])
        assert "8 threads x 1000 lookups over 3 devices x 4 keys: 12 queries, 9 raises, 0 wrong values" in r.stdout
        assert "\n0 failures\n" in r.stdout


def test_the_cache_header_is_plain_cxx_and_the_library_compiles_it():
    core = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "launch_cache_core.h")).read())
    assert not re.search(r"\bhip[A-Z_]\w*|#include\s*<hip|#include\s*\"|__global__|__device__|getenv", core)
    assert "std::mutex" in core and "std::lock_guard" in core
    runtime = open(os.path.join(CSRC, "runtime.cpp")).read()
    lds, slots = (runtime.split("int %s(" % f)[1].split("\n}\n")[0] for f in ("kernel_lds", "kernel_slots"))
    assert '#include "launch_cache_core.h"' in runtime and "hipGetDevice(&dev)" in lds and "g_launch.lds_limit(dev, kernel," in lds
    assert "kernel_lds(kernel, lds)" in slots and "hipGetDevice(&dev)" in slots and "g_launch.slots(dev, kernel," in slots


def test_the_two_runtime_calls_live_in_runtime_cpp_only():
    src = sources()
    for word in ("hipFuncSetAttribute", "hipOccupancyMaxActiveBlocksPerMultiprocessor", "hipOccupancyMax"):
        assert [n for n, text in src.items() if word in text] == ["runtime.cpp"], word
    # no launcher keeps a function-level variable of its own across calls (what is cached is cached per device): an indented
    # `static` declaration of a variable, with no initialiser, `= ...` or `{...}` (one in parentheses reads like a function's
    # declaration and is not told apart), is one of three known names, whatever its type is spelled like
    decl = re.compile(r"^[ \t]+(?:thread_local\s+)?static\s+(?:thread_local\s+)?(?!constexpr\b|const\b|_assert\b)"
                      r"[^;(){}=\n]*?\b(\w+)\s*(?:=[^;\n]*|\{[^;\n]*\})?;", re.M)
    found = {(name, m.group(1)) for name, text in src.items() for m in decl.finditer(text.replace("static_assert", "static _assert"))}
    # (mr_global_plan's locked cache of a rule of the length alone and the pinned result block of a calling thread: neither
    # belongs to a launcher or depends on the device)
    assert found == {("mixed_radix.hip", "mu"), ("mixed_radix.hip", "cache"), ("capi.cpp", "pin")}, found
    probe = "    static int occ = 0;\n    static bool done{false};\n    static  std::map<int, int>  m;\n    static constexpr int K = 3;\n"
    assert [m.group(1) for m in decl.finditer(probe)] == ["occ", "done", "m"]  # (the rule sees what it is meant to see)


def test_the_register_resident_descriptor_is_defined_once():
    src = sources()
    assert [n for n, text in src.items() if re.search(r"\bstruct MrReg3Io\b\s*(\{|$)", text, re.M)] == ["mr_reg_io.h"]
    assert [n for n, text in src.items() if re.search(r"constexpr int MR_REG3_NOT_BUILT\b", text)] == ["mr_reg_io.h"]
    for unit in ("mixed_radix.hip", "mixed_radix_reg3.h", "mixed_radix_reg2.h"):
        assert '#include "mr_reg_io.h"' in src[unit], unit


def test_hdrs_names_every_header_the_units_include():
    src = sources()
    with open(os.path.join(CSRC, "Makefile")) as f:
        hdrs = set(re.search(r"^HDRS = (.*)$", f.read(), re.M).group(1).split())
    # a unit's headers include headers of their own: follow them
    seen, todo = set(), [n for n in src if n.endswith((".hip", ".cpp"))]
    while todo:
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', src[todo.pop()], re.M):
            if inc not in seen:
                seen.add(inc)
                if inc in src:
                    todo.append(inc)
    assert seen and not sorted(seen - hdrs), sorted(seen - hdrs)
    assert {"launch_cache_core.h", "mr_reg_io.h"} <= seen
