"""The call scaffold of p2s_devcall.h (PoolScratch, Carver, DEV_CHECK, dev_oom, select_device, blocks, until_unchanged) against
a fake of the block cache and of the runtime calls it makes that records their order: tests/devcall_host_test.cpp, a stand-alone
host program, built with the address and undefined-behaviour sanitizers and run.  No GPU, no HIP headers."""
import os
import subprocess

import pytest

from test_devmem_host import host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))


def test_scaffold_drains_then_frees_exactly_once(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'devcall_host_test')
    subprocess.run([cxx, '-std=c++17', '-Wall', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    os.path.join(HERE, 'devcall_host_test.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'devcall host test ok' in run.stdout
