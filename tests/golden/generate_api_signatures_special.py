"""Build container only: record the public names and call signatures of the reference's two liquid-crystal waveguide
modules (spomso.cores.geom_vector_special, vector_functions_special) as JSON, in the format of
generate_api_signatures.py, so that tests/test_lcwg_cpu.py can check the mirror where the reference is absent.

    PYTHONPATH=/root/reference/Code/spomso python tests/golden/generate_api_signatures_special.py
"""
import importlib
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from generate_api_signatures import describe  # noqa: E402  (puts the reference on sys.path)

MODULES = ["geom_vector_special", "vector_functions_special"]


def main():
    rec = {"modules": {m: describe(importlib.import_module("spomso.cores." + m)) for m in MODULES}}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_api_special.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(path, sum(len(v) for v in rec["modules"].values()), "names")


if __name__ == "__main__":
    main()
