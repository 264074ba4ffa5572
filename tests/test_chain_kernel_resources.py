"""The screened chain kernel p2s_chain_kernel<false, true> keeps its register budget: no scratch, no spilled VGPR, at most 256
VGPRs, two waves per SIMD (two workgroups per CU).

The kernel sits at the edge of the 256 registers two workgroups per CU leave it: the depth of the confirm's load pipeline
(SCR_CDEPTH) and the per-tile rebuilding of its per-lane addresses were chosen from the compiler's resource report
(profiles/r10/kernel_resources.txt), and a change of the kernel or of the compiler can bring spills back without any result
changing.  This compiles the device code of p2s_chain.hip with the build's own flags and reads the report; no GPU is needed."""
import os
import re
import subprocess

from points2surf_amd import build as b

SCREENED = 'p2s_chain_kernelILb0ELb1E'        # p2s_chain_kernel<false, true> in the mangled name


def _report():
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
    return fields


def test_screened_kernel_has_no_scratch_and_two_workgroups_per_cu():
    rep = _report()
    names = [n for n in rep if SCREENED in n]
    assert len(names) == 1, sorted(rep)
    r = rep[names[0]]
    print(r)
    assert int(r['ScratchSize [bytes/lane]']) == 0
    assert int(r['VGPRs Spill']) == 0
    assert int(r['VGPRs']) + int(r['AGPRs']) <= 256
    assert int(r['Occupancy [waves/SIMD]']) == 2
