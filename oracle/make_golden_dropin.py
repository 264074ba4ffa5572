"""TEST INFRASTRUCTURE ONLY -- write tests/golden/ref_dropin_outputs.json: what the UNMODIFIED reference's own
``parse_arguments``, ``eval_predictions`` and ``mesh_comparison`` return / write for the inputs of
tests/test_dropin_api.py and tests/test_dropin_reports.py, so that those tests also run where no reference checkout
exists.  Run where one does (P2S_REFERENCE_ROOT):

    python -m oracle.make_golden_dropin
"""
import importlib.util
import json
import os
import sys
import tempfile
import pathlib

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DROPIN = os.path.join(REPO, 'points2surf_amd', 'dropin')
OUT = os.path.join(REPO, 'tests', 'golden', 'ref_dropin_outputs.json')


def _test_module(name):
    spec = importlib.util.spec_from_file_location('_golden_' + name, os.path.join(REPO, 'tests', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _drop_source_modules():
    for k in [k for k in sys.modules if k == 'source' or k.startswith('source.')]:
        del sys.modules[k]


def parse_arguments_outputs(api):
    from oracle import ref_shims
    _drop_source_modules()
    with ref_shims.reference():
        from source import points_to_surf_eval as ref_ev
        out = {'defaults': vars(ref_ev.parse_arguments([])), 'args': vars(ref_ev.parse_arguments(api.PARSE_ARGS))}
    _drop_source_modules()
    return json.loads(json.dumps(out))


def report_outputs(rep):
    from oracle import ref_shims
    _drop_source_modules()
    sys.path.insert(0, ref_shims.REFERENCE_ROOT)
    sys.path.insert(0, DROPIN)
    mp = pytest.MonkeyPatch()
    try:
        import source.base.evaluation as ours
        ref = ours._ref
        assert ref is not None and ref.__file__.startswith(ref_shims.REFERENCE_ROOT)
        out = {'eval_predictions': {}}
        with tempfile.TemporaryDirectory() as tmp:
            tmp = pathlib.Path(tmp)
            pred, gt = rep.eval_predictions_inputs(tmp)
            for unsigned in (False, True):
                out['eval_predictions']['unsigned' if unsigned else 'signed'] = rep.eval_predictions_report(
                    ref, pred, gt, str(tmp / ('ref_%d.csv' % unsigned)), unsigned)
        with tempfile.TemporaryDirectory() as tmp:
            tmp = pathlib.Path(tmp)
            new_dir, ref_dir, ds = rep.mesh_comparison_inputs(tmp)
            rep.patch_reference_mesh_distances(ref, mp)
            text = rep.reference_mesh_comparison_report(ref, new_dir, ref_dir, ds, str(tmp / 'ref.csv'))
            out['mesh_comparison'] = text.replace(str(tmp), '<tmp>')        # the report names the mesh files by path
        return out
    finally:
        mp.undo()
        sys.path.remove(DROPIN)
        sys.path.remove(ref_shims.REFERENCE_ROOT)
        _drop_source_modules()


def main():
    sys.path.insert(0, REPO)
    from oracle import ref_shims
    if not ref_shims.reference_available():
        raise SystemExit('needs a reference checkout (P2S_REFERENCE_ROOT)')
    out = {'parse_arguments': parse_arguments_outputs(_test_module('test_dropin_api'))}
    out.update(report_outputs(_test_module('test_dropin_reports')))
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', OUT)


if __name__ == '__main__':
    main()
