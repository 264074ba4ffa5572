"""The two kernels of a model that reuses the stem keep the register budget of the screened kernel they are built from: no scratch,
no spilled VGPR, at most 256 VGPRs, two waves per SIMD (two workgroups per CU).

p2s_chain_reuse_kernel, the main pass that starts at conv1 from the saved stem, carries 32 more registers than
p2s_chain_kernel<false, true> from the last column tile of a point tile to the next tile's conv1 (the prefetched A fragments
of conv1); p2s_chain_save_kernel, the STN pass that stores them, holds the conv2 weights across conv1
(profiles/r12/kernel_resources.txt).  Like that kernel, both sit at the edge of the 256.  They are kernels of their own names:
the screened kernel must still be found exactly once by its mangled prefix.  The method is that of
tests/test_chain_kernel_resources.py: the device code of p2s_chain.hip compiled with the build's own flags and the compiler's
resource report read; no GPU is needed."""
import os
import re
import subprocess

import pytest

from points2surf_amd import build as b

KERNELS = ('p2s_chain_reuse_kernel', 'p2s_chain_save_kernel')
SCREENED = 'p2s_chain_kernelILb0ELb1E'        # p2s_chain_kernel<false, true> in the mangled name
_CACHE = {}


def _report():
    if 'rep' in _CACHE:
        return _CACHE['rep']
    src = os.path.join(b.CSRC, 'p2s_chain.hip')
    cmd = [b.hipcc_path()] + b._flags() + ['-Rpass-analysis=kernel-resource-usage', '--cuda-device-only', '-c', src, '-o', os.devnull]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stderr[-2000:]
    fields, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r'remark:.*?Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            fields[name] = {}
            continue
        m = re.search(r'remark:\s*(?:\S+:\d+:\d+:)?\s*([A-Za-z][A-Za-z /\[\]]*?):\s*(\S+)\s*\[-Rpass-analysis', line)
        if m and name is not None:
            fields[name][m.group(1).strip()] = m.group(2)
    _CACHE['rep'] = fields
    return fields


@pytest.mark.parametrize('kernel', KERNELS)
def test_kernel_has_no_scratch_and_two_workgroups_per_cu(kernel):
    rep = _report()
    names = [n for n in rep if kernel in n]
    assert len(names) == 1, sorted(rep)
    r = rep[names[0]]
    print(r)
    assert int(r['ScratchSize [bytes/lane]']) == 0
    assert int(r['VGPRs Spill']) == 0
    assert int(r['VGPRs']) + int(r['AGPRs']) <= 256
    assert int(r['Occupancy [waves/SIMD]']) == 2


def test_screened_kernel_is_still_one_instantiation():
    rep = _report()
    assert len([n for n in rep if SCREENED in n]) == 1, sorted(rep)
