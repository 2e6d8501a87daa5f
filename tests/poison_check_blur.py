"""Run by tests/test_blur_gpu.py in a child process with VSD_POISON=1, beside tests/poison_check.py: the engine cases of
tests/blur_cases.py (`edge_blur` with either edge op, `mask_feather`) while every buffer the engine allocates "uninitialised" starts as
0xFF bytes.  Prints one JSON line: a digest of every result; the parent holds them to the digests of its own, unpoisoned runs."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import blur_cases as BC
    import keep_mask_cases as KM
    from videosd_amd import ops as O

    assert O.POISON or os.environ.get("VSD_POISON_CHECK_ANYWAY"), "run with VSD_POISON=1"
    eng = BC.make_engine()
    out = {f"{mode}_{H}x{W}": BC.digest(BC.edge_case(eng, mode, H, W)) for mode, H, W in BC.EDGE_CASES}
    out["feather"] = BC.digest(BC.feather_case(eng, KM.engine_masks(BC.B, 64, 64)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
