"""Recipe and fixture stay together: every runnable generator under oracle/ is run against the imported reference, in a fresh interpreter (the reference's
environment registry and the recorder's patch of torch.optim.Adam.step are process-global) and into a temporary directory, and every file it writes must equal
the committed tests/golden/*.npz: the same keys and, per key, the same dtype, shape and bytes.  No tolerance.  CPU only; the whole module is skipped where the
reference cannot be imported (oracle/_golden_record.reference_root: $SRL_REFERENCE)."""
import glob
import importlib.machinery
import lzma
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ORACLE = os.path.join(ROOT, "oracle")
if ORACLE not in sys.path:
    sys.path.insert(0, ORACLE)

import _golden_record  # noqa: E402
from golden_fixtures import FIXTURES  # noqa: E402

try:
    REFERENCE = _golden_record.reference_root()
except SystemExit as e:
    pytest.skip(f"the reference cannot be imported: {e}", allow_module_level=True)
if importlib.machinery.PathFinder.find_spec("srl", [REFERENCE]) is None or importlib.machinery.PathFinder.find_spec("torch") is None:
    pytest.skip(f"the reference cannot be imported: no srl package under {REFERENCE}, or no torch", allow_module_level=True)


def _state_dict_of(parameter_file):
    """The reference's parameter file (srl/utils/common.py:117-134): an lzma container of a pickled state_dict."""
    sd = pickle.loads(lzma.decompress(parameter_file.tobytes()))
    return [(k, str(v.dtype), tuple(v.shape), v.numpy().tobytes()) for k, v in sd.items()]


# Run, but not compared byte for byte: {fixture: (array, or None for the whole file; reason; what is compared exactly in the array's place, or None)}.
# Only actor_priority_n3, ppo_v_step_discrete and f1_parameter_dqn may ever stand here: the three fixtures that their recipes did not reproduce before the
# recipes seeded torch, numpy and random ahead of the first network of the process.
NOT_COMPARED = {
    "f1_parameter_dqn": ("parameter_file", "the reference pickles torch tensors, and torch's pickle names every storage by its address in the writing process "
                         "(the digits after `FloatStorage` in the decompressed file): the bytes differ from run to run where the weights do not.  The decoded "
                         "state_dict is compared instead, exactly; `q`, `probe` and `keys` of the same file are compared like every other array.", _state_dict_of),
}

CHILD_TIMEOUT_S = 300  # the generators take 1 to 12 s each


def test_every_fixture_has_exactly_one_recipe(golden_dir):
    claimed = [name for names in FIXTURES.values() for name in names]
    twice = sorted({n for n in claimed if claimed.count(n) > 1})
    committed = sorted(os.path.basename(p)[: -len(".npz")] for p in glob.glob(os.path.join(golden_dir, "*.npz")))
    assert not twice, f"claimed by more than one generator: {twice}"
    assert sorted(claimed) == committed, f"unclaimed: {sorted(set(committed) - set(claimed))}, claimed but not committed: {sorted(set(claimed) - set(committed))}"
    assert all(os.path.isfile(os.path.join(ORACLE, g)) for g in FIXTURES)
    assert set(NOT_COMPARED) <= {"actor_priority_n3", "ppo_v_step_discrete", "f1_parameter_dqn"} and all(reason for _, reason, _ in NOT_COMPARED.values())


@pytest.mark.parametrize("generator", sorted(FIXTURES))
def test_recipe_reproduces_its_fixtures(generator, tmp_path, golden_dir):
    env = dict(os.environ, SRL_REFERENCE=REFERENCE, PYTHONDONTWRITEBYTECODE="1")
    run = subprocess.run([sys.executable, os.path.join(ORACLE, generator), str(tmp_path)], env=env, cwd=str(tmp_path), timeout=CHILD_TIMEOUT_S,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npz" for n in FIXTURES[generator]), "the generator wrote other files than the table says"
    differing = {}
    for name in FIXTURES[generator]:
        skip, _, instead = NOT_COMPARED.get(name, ("", "", None))
        if skip is None:
            continue
        got, want = np.load(tmp_path / (name + ".npz"), allow_pickle=False), np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
        assert sorted(got.files) == sorted(want.files), name
        bad = [k for k in want.files if k != skip and (got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes())]
        if instead is not None and instead(got[skip]) != instead(want[skip]):
            bad.append(skip + " (decoded)")
        if bad:
            differing[name] = f"{len(bad)} of {len(want.files)} arrays, first {bad[:3]}"
    assert not differing, differing
