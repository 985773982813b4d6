"""Records the conv / GEMM launcher's decision for every problem of tests/conv_plan_cases.py into tests/golden/conv_plan_table.npz.

    python tests/golden/make_conv_plan_table.py

The committed table was recorded at commit 691758c ("Run v-prediction / SD-2.x models"), BEFORE the launcher's decision code was
reorganised into one planner: it pins what that commit decided, so that the refactor (and every later change that does not mean to
move a decision) can be checked case by case on a CPU.  Re-record only when a decision is changed on purpose, and say which.

The file holds `outcomes` (the distinct (kind, form, split, narrow) tuples, int16 [k, 4]; a refusal is (-1, 0, 0, 0)), `index` (uint8 [n]:
the outcome of every case, in generator order), `block_names` / `block_sizes`, and `cases_sha256` (hash of the generated case list).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import conv_plan_cases as cases  # noqa: E402


def main():
    from distdiff_amd import _lib
    _lib.lib()
    blks = list(cases.blocks())
    res = np.concatenate([cases.evaluate(_lib.LIB_PATH, rows) for _name, rows in blks])
    outcomes, index = np.unique(res, axis=0, return_inverse=True)
    assert len(outcomes) < 256
    path = os.path.join(HERE, "conv_plan_table.npz")
    np.savez_compressed(path, outcomes=outcomes.astype(np.int16), index=index.reshape(-1).astype(np.uint8),
                        block_names=np.array([n for n, _r in blks]), block_sizes=np.array([len(r) for _n, r in blks], dtype=np.int64),
                        cases_sha256=np.array(cases.cases_hash(blks)))
    print("%d cases, %d outcomes, %d bytes -> %s" % (len(res), len(outcomes), os.path.getsize(path), path))
    kinds, counts = np.unique(res[:, 0], return_counts=True)
    print("cases per kind:", dict(zip(kinds.tolist(), counts.tolist())))


if __name__ == "__main__":
    main()
