"""Re-record ``tests/golden/reference/*.npz``: the reference's side of the value comparisons in tests/test_seam_cpu.py and
tests/test_data_cpu.py (generator streams, reset / stepped states, PPO-style re-evaluation, instance files, augmentations,
the POMO epilogue), computed by the reference's own code through ``oracle/ref_import.py`` (needs its checkout).

    python -m oracle.gen_reference_records

Runs those tests with ``RL4CO_RECORD_REFERENCE=1``: every ``tests.helpers.reference_record(key, compute)`` runs ``compute``
and writes its record, then the test compares the product against it as it does everywhere else.
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

RECORDED = {
    "tests/test_seam_cpu.py": ["test_ppo_style_reevaluation_matches_reference_policy", "test_product_generators_follow_the_reference_stream",
                               "test_reset_state_has_the_reference_keys_and_dtypes", "test_stepped_state_matches_the_reference_key_by_key"],
    "tests/test_data_cpu.py": ["test_dihedral8_matches_reference_transform", "test_state_augmentation_matches_reference_transform",
                               "test_pomo_best_restatement_equals_reference_epilogue", "test_generated_instance_files_equal_reference_generator",
                               "test_generate_dataset_files_equal_reference"],
}


def main() -> None:
    from oracle import ref_import

    if not ref_import.available():
        raise SystemExit(f"reference checkout not found under {ref_import.REFERENCE_ROOT} (RL4CO_REFERENCE_ROOT)")
    ids = [f"{path}::{name}" for path, names in RECORDED.items() for name in names]
    env = dict(os.environ, RL4CO_RECORD_REFERENCE="1")
    rc = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", *ids], cwd=ROOT, env=env).returncode
    raise SystemExit(rc)


if __name__ == "__main__":
    main()
