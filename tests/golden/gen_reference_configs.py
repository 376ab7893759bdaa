"""Fingerprints of the reference's layer-selection configs.

    python tests/golden/gen_reference_configs.py REFERENCE_ROOT      # a checkout of the reference project; writes tests/golden/reference_configs.json

For every `feature/configs/*.json` of the reference: the sha256 of its parsed {id: bool} content re-serialised with json.dumps
(key order kept) and its number of ids.  test_every_layer_config_of_the_reference_is_served holds the shipped configs to these."""
import glob
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def fingerprint(path):
    cfg = json.load(open(path))
    return {"sha256": hashlib.sha256(json.dumps(cfg).encode()).hexdigest(), "ids": len(cfg)}


def main(ref_root):
    files = sorted(glob.glob(os.path.join(ref_root, "feature", "configs", "*.json")))
    assert files, "reference configs not found"
    out = {os.path.basename(f): fingerprint(f) for f in files}
    with open(os.path.join(HERE, "reference_configs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(out), "configs")


if __name__ == "__main__":
    main(sys.argv[1])
