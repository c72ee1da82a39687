"""The device forms of include/glabc_numerics.h are what an offline gfx950 build compiles (tests/test_hip_boxmuller.py pins
their bits, and would pass on the host text as well): the disassembly of glabc_normal_pair applies the quadrant's signs
with v_bitop3_b32, and goes back to the host text, which has no three-input bit operation, under -DGLABC_HOST_TEXT.  Cross-compiles; no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = r'''
#include <hip/hip_runtime.h>
#include "glabc_numerics.h"
extern "C" __global__ void k(const uint32_t* in, float* out)
{
    float z0, z1;
    glabc_normal_pair(in[2 * threadIdx.x], in[2 * threadIdx.x + 1], &z0, &z1);
    out[2 * threadIdx.x] = z0;
    out[2 * threadIdx.x + 1] = z1;
}
'''


def _asm(tmp_path, *flags):
    src = tmp_path / "pair.hip"
    src.write_text(SRC)
    out = tmp_path / "pair.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                           "-I", os.path.join(ROOT, "include"), *flags, str(src), "-o", str(out)])
    return out.read_text()


def test_offline_device_build_compiles_the_device_forms(tmp_path):
    dev = _asm(tmp_path)
    host = _asm(tmp_path, "-DGLABC_HOST_TEXT")
    assert dev.count("v_bitop3_b32") == 2 and "v_bitop3_b32" not in host
    n_dev = sum(1 for l in dev.splitlines() if l.strip().startswith("v_"))
    n_host = sum(1 for l in host.splitlines() if l.strip().startswith("v_"))
    assert n_dev < n_host, (n_dev, n_host)
