"""The argument blocks of the kernels (heyoka_amd/csrc/kernel_args.hpp): the host struct and the device text of a block come
from one field list, and here the compiler confirms that the two sides agree - tests/cpp/test_kernel_args.cpp compiles one
empty kernel per block over the device text (hiprtc cross-compiles, no GPU) and prints sizeof of the host struct; the size of
the kernel's argument segment in the metadata of the code object must be that number."""
import os
import re
import subprocess

import pytest

from heyoka_amd import codegen_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "heyoka_amd", "csrc", "_build", "test_kernel_args")

# Every kernel of the library takes one of these (device-side names).
BLOCKS = {"hy_kargs", "hy_dout_args", "hy_grid_args", "hy_ev_stop_args", "hy_doutc_args", "hy_drow_args", "hy_copy_args",
          "hy_ar_kargs", "hy_ed_args", "hy_ep_args", "hy_evr_args", "hy_eva_args", "hy_sa_args", "hy_tmap_args",
          "hy_tmap_cloud_args", "hy_cf_args", "hy_cout_args"}


def _readelf():
    objdump = codegen_check.find_objdump()
    readelf = os.path.join(os.path.dirname(objdump), "llvm-readelf") if objdump else None
    return readelf if readelf and os.path.exists(readelf) else None


def _build_cpp():
    """tests/cpp/test_kernel_args.cpp, compiled the way tests/test_step_action.py compiles its program."""
    src = os.path.join(ROOT, "tests", "cpp", "test_kernel_args.cpp")
    hdr = os.path.join(ROOT, "heyoka_amd", "csrc", "kernel_args.hpp")
    lib = os.path.join(ROOT, "heyoka_amd", "libheyoka_amd.so")
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(src), os.path.getmtime(hdr), os.path.getmtime(lib)):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "heyoka_amd", "csrc"), src,
         "-o", EXE, "-L" + os.path.join(ROOT, "heyoka_amd"), "-lheyoka_amd", "-Wl,-rpath," + os.path.join(ROOT, "heyoka_amd"),
         "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_host_and_device_argument_blocks_have_one_size(tmp_path):
    readelf = _readelf()
    if readelf is None:
        pytest.skip("llvm-readelf not found")
    co = str(tmp_path / "kernel_args.co")
    out = subprocess.run([_build_cpp(), co], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    host = {dev: int(size) for dev, size in (line.split() for line in out.stdout.splitlines())}
    assert set(host) == BLOCKS and len(out.stdout.splitlines()) == len(BLOCKS), sorted(host)
    notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
    # One block per kernel, fields sorted alphabetically (see codegen_check.kernel_resources()).
    device = {}
    for b in re.split(r"\n\s+- \.agpr_count:", "\n" + notes)[1:]:
        name = re.search(r"\.name:\s+k_(\S+)", b)
        size = re.search(r"\.kernarg_segment_size:\s+(\d+)", b)
        assert name and size, b
        device[name.group(1)] = int(size.group(1))
    print(sorted(device.items()))
    assert device == host
