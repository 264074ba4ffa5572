"""The owners of p2s_devmem.h (DevBuf, PinnedBuf, DevEvent, DevStream, p2s_alloc_all) against a counting fake of the HIP
calls they make: tests/devmem_host_test.cpp, a stand-alone host program, built with the address and undefined-behaviour
sanitizers and run.  No GPU, no HIP headers."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def host_compiler():
    for cxx in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_owners_free_exactly_once(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'devmem_host_test')
    subprocess.run([cxx, '-std=c++17', '-Wall', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    os.path.join(HERE, 'devmem_host_test.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'devmem host test ok' in run.stdout
