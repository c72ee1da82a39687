"""Compiler resource report of the run-time compiled predictive kernel (glabc_rtc_compile_predictive): registers, private segment and
spills of predictive_kernel<D, YD, R> around the Mixture restatement, the test sources and the Lotka-Volterra example, at the rule
R = 1 and -- for the two sources the rule was weighed on -- at the built-in kernels' R = 16 / D (GLABC_RTC_PRED_ROWS).  hiprtc
cross-compiles without a GPU (the compile then ends in GLABC_ERR_NO_DEVICE, after the log is written); GLABC_RTC_OPTS adds
-Rpass-analysis=kernel-resource-usage to the library's own options, and the kernel's remarks are taken from the log, with the
seconds the compile took.  The kernel's code size is its symbol's size in the code object, which GLABC_RTC_DUMP writes beside the
translation unit and llvm-readelf reads.

    python tools/rtc_predictive_resources.py > profiles/rtc_predictive_kernel_resources.txt
"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-abc-mcmc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["GLABC_RTC_OPTS"] = "-Rpass-analysis=kernel-resource-usage"
from glabcmcmc_amd import _capi  # noqa: E402
from glabcmcmc_amd.examples import LotkaVolterra_smc  # noqa: E402
from test_rtc import ALL_USER, NONLINEAR, mixture_source  # noqa: E402
from test_rtc_draws_host import DIS_AND_KERNEL  # noqa: E402

EDGE = {}
with open(os.path.join(ROOT, "tests", "test_rtc_draws_shapes.py")) as f:
    text = f.read()
for name in ("EDGE1", "EDGE8"):
    EDGE[name] = re.search(name + r' = """(.*?)"""', text, re.S).group(1)

MIXTURE = ("Mixture restated (2, 2, 2)", mixture_source([0.05 ** 0.5] * 2), (2, 2, 2))
LV = ("examples/LotkaVolterra_smc.py (2, 8, 8)", LotkaVolterra_smc.SOURCE, (2, 8, 8))
READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
SOURCES = [MIXTURE + (1,), MIXTURE + (2,), MIXTURE + (8,), LV + (1,), LV + (2,), LV + (8,), ("NONLINEAR (3, 2, 4)", NONLINEAR, (3, 2, 4), 1),
           ("user discrepancy and kernel (2, 3, 3)", DIS_AND_KERNEL, (2, 3, 3), 1), ("every callback the user's (2, 3, 3)", ALL_USER, (2, 3, 3), 1),
           ("edge (1, 1, 1)", EDGE["EDGE1"], (1, 1, 1), 1), ("edge (8, 8, 5)", EDGE["EDGE8"], (8, 8, 5), 1)]
KEEP = ("Function Name", "TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size")


def code_bytes(code_object):
    """the size of predictive_kernel's symbol in the code object, in bytes of instructions"""
    out = subprocess.run([READELF, "-sW", code_object], capture_output=True, text=True, check=True).stdout
    sizes = {int(f[2]) for f in (line.split() for line in out.splitlines()) if len(f) >= 8 and f[3] == "FUNC" and "predictive_kernel" in f[7]}
    assert len(sizes) == 1, out
    return sizes.pop()


def main():
    lib = _capi.lib()
    dump = os.path.join(tempfile.mkdtemp(), "unit.hip")
    os.environ["GLABC_RTC_DUMP"] = dump
    for name, source, dims, rows in SOURCES:
        os.environ["GLABC_RTC_PRED_ROWS"] = str(rows)
        handle, log = C.c_void_p(), C.create_string_buffer(1 << 18)
        t0 = time.time()
        rc = lib.glabc_rtc_compile_predictive(source.encode(), *dims, C.byref(handle), log, len(log))
        seconds = time.time() - t0
        assert rc in (0, -6), (rc, log.value.decode()[:2000])
        if rc == 0:
            lib.glabc_rtc_release(handle)
        print("## %s, R = %d rows per item (the whole program compiled in %.1f s)" % (name, rows, seconds))
        print("    Code size [bytes]: %d" % code_bytes(dump + ".co"))
        show = False
        for line in log.value.decode().splitlines():
            if "note: predictive_kernel" in line:
                print(line)
            m = re.search(r"remark: (.*?) \[-Rpass-analysis", line)
            if not m:
                continue
            body = m.group(1)
            if body.startswith("Function Name"):
                show = "predictive_kernel" in body
            if show and body.strip().startswith(KEEP):
                print(body)


if __name__ == "__main__":
    main()
