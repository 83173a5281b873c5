"""Golden composition of the REFERENCE's own configs/ tree, written to tests/golden/reference_configs.json.

    python oracle/make_config_goldens.py <reference checkout>/configs

The composer (multimodalanalytical_amd/config.py) is pointed at the reference's configs/ tree, unchanged, with the override
lists of tests/test_config_cpu.py (the reference test's list, tests/test_run.py:8-18, and the groups of its mixture runs); the
composed configs are stored as JSON.  The fixture travels with the repository, so tests/test_config_cpu.py compares this
repo's configs/ against it without the reference tree.  TEST INFRASTRUCTURE ONLY.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodalanalytical_amd.config import compose  # noqa: E402
from tests.test_config_cpu import C5, OVERRIDES  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_configs.json")


def main(ref_configs):
    if not os.path.isfile(os.path.join(ref_configs, "config_train.yaml")):
        raise SystemExit(f"{ref_configs}: not a configs/ tree (no config_train.yaml)")
    cases = {"test_run_overrides": OVERRIDES, "mixture_run_groups": C5}
    out = {name: {"overrides": ov, "config": compose(ref_configs, "config_train", ov)} for name, ov in cases.items()}
    for v in out.values():
        assert json.loads(json.dumps(v["config"])) == v["config"], "composed config does not survive JSON"
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
