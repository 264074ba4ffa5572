"""The small layers of the chain kernels (K = 64, v_mfma_f32_32x32x2_f32) have their operands requested ahead of the MFMAs that
use them: few full waits stand directly in front of an MFMA, and conv1 of p2s_chain_reuse_kernel requests
its eight W1' fragments before its first MFMA.

Left to itself the scheduler moved every request of a K = 64 layer directly in front of the four MFMAs that use it, whatever
order the source had: one `s_waitcnt lgkmcnt(0)` per k-group in conv0b, conv1 and conv2, and in the reuse kernel one
buffer_load_dwordx4 of W1' -> `s_waitcnt vmcnt(0)` -> four MFMAs, seven times per tile.  Scheduling fences in layer_k64 and
around the reuse kernel's conv1 keep the source's order; nothing in a result shows whether they still do after a change of the
kernels or of the compiler, so this compiles the device code of p2s_chain.hip to assembly with the build's own flags (as
tests/test_chain_kernel_resources.py obtains its report) and looks at the waits and the MFMAs only.  No GPU is needed.

Counted per kernel: the full waits -- `s_waitcnt vmcnt(0)` or `s_waitcnt lgkmcnt(0)` alone on the line -- whose next
instruction is a v_mfma_f32_32x32x2_f32.  What remains is the last k-group of a layer (nothing is left to request behind its
operand) and the dense conv3's pipeline, which this change does not touch (profiles/r14/kernel_resources.txt lists them)."""
import os
import re
import shutil
import subprocess

import pytest

from points2surf_amd import build as b

MFMA = 'v_mfma_f32_32x32x2_f32'
# kernel (part of the mangled name): full waits in front of an MFMA in this build.
# The build before the fences had 36 / 36 / 16 / 36 / 33; the fences alone give 14 / 14 / 9 / 15 / 14, the bound set for them
BOUND = {
    'p2s_chain_kernelILb0ELb0E': 14,      # p2s_chain_kernel<false, false>: dense conv3, max pool
    'p2s_chain_kernelILb0ELb1E': 14,      # p2s_chain_kernel<false, true>: screened
    'p2s_chain_kernelILb1ELb0E': 9,       # p2s_chain_kernel<true, false>: sum pool
    'p2s_chain_save_kernel': 15,
    'p2s_chain_reuse_kernel': 13,
}
_CACHE = {}

pytestmark = pytest.mark.skipif(not (os.path.isfile(b.hipcc_path()) or shutil.which(b.hipcc_path())), reason='no hipcc')


def _kernels():
    """{mangled kernel name: [instruction, ...]} of p2s_chain.hip's device code (labels, directives and comments dropped)"""
    if 'asm' not in _CACHE:
        src = os.path.join(b.CSRC, 'p2s_chain.hip')
        cmd = [b.hipcc_path()] + b._flags() + ['--cuda-device-only', '-S', src, '-o', '-']
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert p.returncode == 0, p.stderr[-2000:]
        out, cur = {}, None
        for line in p.stdout.splitlines():
            s = line.strip()
            m = re.match(r'^(_Z\w+):', s)
            if m:
                cur = out.setdefault(m.group(1), [])
                continue
            if s.startswith('.Lfunc_end'):
                cur = None
                continue
            if cur is None or not s or s[0] in ';.' or s.endswith(':'):
                continue
            cur.append(re.sub(r'\s+', ' ', s.split(';')[0].strip()))
        _CACHE['asm'] = out
    return _CACHE['asm']


def _kernel(part):
    names = [n for n in _kernels() if part in n]
    assert len(names) == 1, sorted(_kernels())
    return _kernels()[names[0]]


def _full_wait(ins):
    return re.fullmatch(r's_waitcnt (vmcnt|lgkmcnt)\(0\)', ins) is not None


@pytest.mark.parametrize('kernel', sorted(BOUND))
def test_full_waits_in_front_of_small_layer_mfmas(kernel):
    ins = _kernel(kernel)
    n = sum(1 for i in range(1, len(ins)) if ins[i].startswith(MFMA) and _full_wait(ins[i - 1]))
    print(kernel, n)
    assert n <= BOUND[kernel]


def _conv1_of_reuse_kernel():
    """the waits in front of the eight k-groups of conv1 of p2s_chain_reuse_kernel: the only K = 64 layer of that kernel with one
    row tile -- 32 MFMAs into ONE accumulator, the first of them onto the literal 0 (conv2 alternates two accumulators, the
    dense conv3 four).  Returns, per k-group, the s_waitcnt instructions between the previous MFMA and the k-group's first"""
    ins = _kernel('p2s_chain_reuse_kernel')
    mf = [i for i, s in enumerate(ins) if s.startswith(MFMA)]
    layers = []
    for j, i in enumerate(mf):
        if not ins[i].endswith(', 0'):
            continue
        run = mf[j:j + 32]
        acc = ins[i].split(' ')[1]
        if len(run) == 32 and all(ins[k].split(' ')[1] == acc for k in run) and \
                all(not ins[k].endswith(', 0') for k in run[1:]) and (j + 32 == len(mf) or ins[mf[j + 32]].split(' ')[1] != acc):
            layers.append(run)
    assert len(layers) == 1, [ins[r[0]] for r in layers]
    run = layers[0]
    groups = []
    for g in range(8):
        first = run[4 * g]
        k = first - 1
        w = []
        while k >= 0 and not ins[k].startswith('v_mfma') and first - k < 64:
            if ins[k].startswith('s_waitcnt'):
                w.append(ins[k])
            k -= 1
        groups.append(w)
        # the four MFMAs of a k-group follow each other: nothing is waited for inside a k-group
        assert run[4 * g + 3] - first == 3, (g, ins[first:run[4 * g + 3] + 1])
    return groups


def test_reuse_kernel_requests_w1_before_conv1s_first_mfma():
    """With all eight fragments of W1' requested in front of the first MFMA, the k-groups wait for them in steps -- vmcnt(n) with
    n falling to 0 at the last k-group at the earliest.  A fragment requested between two k-groups shows as a full vmcnt(0) in
    front of the next one (the form before the fences: seven of them)"""
    groups = _conv1_of_reuse_kernel()
    print(groups)
    for g, waits in enumerate(groups[:7]):
        for w in waits:
            m = re.search(r'vmcnt\((\d+)\)', w)
            assert m is None or int(m.group(1)) > 0, (g, w)
    # and the steps are there: every k-group but the last waits for its own fragment, with later ones still in flight
    stepped = [max([int(m.group(1)) for w in waits for m in [re.search(r'vmcnt\((\d+)\)', w)] if m] or [-1]) for waits in groups[:7]]
    assert all(v > 0 for v in stepped), stepped
    assert stepped == sorted(stepped, reverse=True), stepped
