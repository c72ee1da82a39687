#!/usr/bin/env python3
"""What two builds of the library hand to hiprtc for the same arguments: the translation unit, the compiler options and the
first name expression (GLABC_RTC_DUMP), the status and the log of each compile, side by side.  Needs no GPU: hiprtc compiles
without one and the load then fails with GLABC_ERR_NO_DEVICE.

    python tools/rtc_dump_compare.py BEFORE/libglabc_hip.so AFTER/libglabc_hip.so > profiles/NAME.txt

Each library is driven in a process of its own (`--dump LIB DIR`); the parent compares the files the two left."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gl-abc-mcmc_amd"), os.path.join(ROOT, "tests")]
GLMCMC, GLOBAL, GAMMA = 0, 1, 1


def cases():
    from test_rtc import ALL_USER, NONLINEAR, mixture_source
    from test_gamma_models import USER_SRC
    mix = mixture_source((0.2236068, 0.2236068))
    reg = []                       # (name, source, algo, D, YD, ND, N, flags, GLABC_RTC_LANES or None)
    for n in (5, 16):
        reg.append(("glmcmc mixture (2,2,2) N %d" % n, mix, GLMCMC, 2, 2, 2, n, 0, "1"))
    for n in (5, 12):
        for flags in (0, GAMMA):
            reg.append(("glmcmc user (2,3,3) N %d flags %d" % (n, flags), USER_SRC, GLMCMC, 2, 3, 3, n, flags, "1"))
    reg.append(("glmcmc user (2,3,3) N 5 flags 1 lanes 4", USER_SRC, GLMCMC, 2, 3, 3, 5, GAMMA, "4"))
    reg.append(("glmcmc nonlinear (3,2,4) N 13 lanes 2", NONLINEAR, GLMCMC, 3, 2, 4, 13, 0, "2"))
    reg.append(("glmcmc nonlinear (3,2,4) N 13 lanes searched", NONLINEAR, GLMCMC, 3, 2, 4, 13, 0, None))
    reg.append(("globalmcmc mixture (2,2,2)", mix, GLOBAL, 2, 2, 2, 1, 0, "1"))
    reg.append(("globalmcmc mixture (2,2,2) flags 1", mix, GLOBAL, 2, 2, 2, 1, GAMMA, "1"))
    reg.append(("glmcmc all hooks (2,3,3) N 5", ALL_USER, GLMCMC, 2, 3, 3, 5, 0, "1"))
    reg.append(("globalmcmc all hooks (2,3,3)", ALL_USER, GLOBAL, 2, 3, 3, 1, 0, "1"))
    reg.append(("glmcmc broken source", "GLABC_SIMULATOR void glabc_user_simulate(const float* t, const float* e, float* y) { y[0] = ; }",
                GLMCMC, 1, 1, 1, 3, 0, "1"))
    wide = [("wide nonlinear (3,2,4)", NONLINEAR, 3, 2, 4, 0), ("wide nonlinear (3,2,4) flags 1", NONLINEAR, 3, 2, 4, GAMMA),
            ("wide all hooks (2,3,3)", ALL_USER, 2, 3, 3, 0)]
    return reg, wide


def dump(lib_path, out_dir):
    from glabcmcmc_amd import _capi as A
    lib = C.CDLL(lib_path)
    for name in ("glabc_rtc_compile_ex", "glabc_rtc_compile_wide_ex"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = A.ENTRY_POINTS[name]
    reg, wide = cases()
    results = []
    for i, case in enumerate([c + ("reg",) for c in reg] + [c + ("wide",) for c in wide]):
        unit = os.path.join(out_dir, "unit_%02d.hip" % i)
        os.environ["GLABC_RTC_DUMP"] = unit
        handle, log = C.c_void_p(), C.create_string_buffer(1 << 16)
        t0 = time.perf_counter()
        if case[-1] == "reg":
            name, src, algo, d, yd, nd, n, flags, lanes, _ = case
            os.environ.pop("GLABC_RTC_LANES", None)
            if lanes:
                os.environ["GLABC_RTC_LANES"] = lanes
            rc = lib.glabc_rtc_compile_ex(src.encode(), algo, d, yd, nd, n, flags, C.byref(handle), log, len(log))
        else:
            name, src, d, yd, nd, flags, _ = case
            rc = lib.glabc_rtc_compile_wide_ex(src.encode(), d, yd, nd, flags, C.byref(handle), log, len(log))
        results.append(dict(name=name, rc=rc, log=log.value.decode(errors="replace"), seconds=round(time.perf_counter() - t0, 2),
                            unit=open(unit).read() if os.path.exists(unit) else None))
    json.dump(results, open(os.path.join(out_dir, "results.json"), "w"))


def main():
    if sys.argv[1] == "--dump":
        return dump(sys.argv[2], sys.argv[3])
    sides = []
    for lib in sys.argv[1:3]:
        d = tempfile.mkdtemp()
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--dump", os.path.abspath(lib), d])
        sides.append(json.load(open(os.path.join(d, "results.json"))))
    different = 0
    print("# translation unit + options + first name expression (GLABC_RTC_DUMP), status and log of each compile: before | after")
    for a, b in zip(*sides):
        same = a["unit"] == b["unit"] and a["rc"] == b["rc"] and a["log"] == b["log"]
        different += not same
        digest = hashlib.sha256((a["unit"] or "").encode()).hexdigest()[:16]
        defines = [l.split()[1] for l in (a["unit"] or "").splitlines() if l.startswith("#define GLABC_RTC_")]
        print("%-48s %s  status %d | %d  log %d | %d bytes  unit %s %d bytes  %.2f | %.2f s\n    %s\n    %s" % (
            a["name"], "identical" if same else "DIFFERENT", a["rc"], b["rc"], len(a["log"]), len(b["log"]), digest, len(a["unit"] or ""),
            a["seconds"], b["seconds"], (a["unit"] or "\n\n").splitlines()[1], " ".join(defines)))
    print("# %d of %d compiles differ" % (different, len(sides[0])))
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
