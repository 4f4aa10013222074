"""The context's record of its device allocations (csrc/fwi_devmem.h) on the CPU: tests/devmem_host.cpp drives
fwi::DeviceMemory with a fake allocator over malloc -- round trips, pointers moved inside their allocation, null and
foreign pointers, a failed allocation in mid-sequence, release_all with swapped slots and refused frees, growth -- built
with the address and undefined-behaviour sanitizers as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_memory_record_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/devmem_host.cpp")
    exe = str(tmp_path / "devmem_host")
    # (the sanitizers' runtimes inside the program: it then runs as it is, whatever else the loader brings along)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-static-libasan",
                           "-static-libubsan", "-g",
                           "-I", os.path.join(ROOT, "full_waveform_inversion_amd", "csrc"),
                           os.path.join(ROOT, "tests", "devmem_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
