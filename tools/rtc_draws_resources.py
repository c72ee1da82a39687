"""Compiler resource report of the run-time compiled draw kernels (glabc_rtc_compile_draws): registers, private segment and spills of
abc_draws_kernel / smc_draws_kernel around the test sources and the Lotka-Volterra example.  hiprtc cross-compiles without a GPU
(the compile then ends in GLABC_ERR_NO_DEVICE, after the log is written); GLABC_RTC_OPTS adds -Rpass-analysis=kernel-resource-usage
to the library's own options, and the remarks of the two draw kernels are taken from the log.

    python tools/rtc_draws_resources.py > profiles/rtc_draws_kernel_resources.txt
"""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-abc-mcmc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["GLABC_RTC_OPTS"] = "-Rpass-analysis=kernel-resource-usage"
from glabcmcmc_amd import _capi  # noqa: E402
from glabcmcmc_amd.examples import LotkaVolterra_smc  # noqa: E402
from test_rtc import NONLINEAR, mixture_source  # noqa: E402
from test_rtc_draws_host import DIS_AND_KERNEL  # noqa: E402

EDGE = {}
with open(os.path.join(ROOT, "tests", "test_rtc_draws_shapes.py")) as f:
    text = f.read()
for name in ("EDGE1", "EDGE8"):
    EDGE[name] = re.search(name + r' = """(.*?)"""', text, re.S).group(1)

SOURCES = [("Mixture restated (2, 2, 2)", mixture_source([0.05 ** 0.5] * 2), (2, 2, 2)), ("NONLINEAR (3, 2, 4)", NONLINEAR, (3, 2, 4)),
           ("user discrepancy and kernel (2, 3, 3)", DIS_AND_KERNEL, (2, 3, 3)), ("edge (1, 1, 1)", EDGE["EDGE1"], (1, 1, 1)),
           ("edge (8, 8, 5)", EDGE["EDGE8"], (8, 8, 5)), ("examples/LotkaVolterra_smc.py (2, 8, 8)", LotkaVolterra_smc.SOURCE, (2, 8, 8))]
KEEP = ("Function Name", "TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size")


def main():
    lib = _capi.lib()
    print("# Compiler resource report of the run-time compiled draw kernels (glabc_rtc_compile_draws, csrc/glabc_rtc.hip; gfx950): what\n"
          "# -Rpass-analysis=kernel-resource-usage prints when hiprtc compiles abc_draws_kernel<D, YD> (csrc/glabc_abc.h) and\n"
          "# smc_draws_kernel<D, YD> (csrc/glabc_smc.h) around a user's source with the library's options (--offload-arch=gfx950 -O3\n"
          "# -std=c++17 -ffp-contract=off -fno-slp-vectorize).  (theta_dim, y_dim, noise_dim) after each name.  ScratchSize is the private\n"
          "# segment in bytes per lane.  Written by tools/rtc_draws_resources.py; the row kernels of the programs are left out.")
    for name, source, dims in SOURCES:
        handle, log = C.c_void_p(), C.create_string_buffer(1 << 18)
        rc = lib.glabc_rtc_compile_draws(source.encode(), *dims, C.byref(handle), log, len(log))
        assert rc in (0, -6), (rc, log.value.decode()[:2000])
        if rc == 0:
            lib.glabc_rtc_release(handle)
        print("## %s" % name)
        show = False
        for line in log.value.decode().splitlines():
            m = re.search(r"remark: (.*?) \[-Rpass-analysis", line)
            if not m:
                continue
            body = m.group(1)
            if body.startswith("Function Name"):
                show = "draws_kernel" in body
            if show and body.strip().startswith(KEEP):
                print(body)


if __name__ == "__main__":
    main()
