"""Records the attention launcher's decision for every problem of tests/attention_plan_cases.py into tests/golden/attention_plan_table.npz.

    python tests/golden/make_attention_plan_table.py

This script asks the library's planner (dd_op_attention_plan).  The COMMITTED table was not made that way: it was recorded at commit
cbe2388 ("Conv/GEMM launcher: one planner, ..."), before the attention dispatch was reorganised into one planner, from that commit's own
dispatch code.  Its attention.hip, attention_shortk.hip and attention_gemm.hip were compiled unchanged, except for a header included
behind kernels.h that redefines hipLaunchKernelGGL to note (kernel stub address, grid, block, dynamic LDS) and hipGetLastError() to
hipSuccess, together with a main() that fills AttnParams as attention_plan_cases.evaluate does and calls launch_attention_fwd / _bwd
(launch_attention_gemm_fwd / _bwd against stubs of launch_conv_gemm / launch_copy_bf16; the images per group are the rows of the first K
copy over Nk).  The stub addresses were resolved through `nm -C`, which keeps the kernels' template arguments: they are the form columns.
Two things are not reachable that way and were carried as literal copies: the engine's choice between the GEMM launcher and the flash
launcher (engine_exec.cpp: attention_gemm_supported(p) && tap1x1 && attention_gemm_workspace(Nq, Nk, D, bwd) <= scratch bytes), and the
GEMM route reports route and group only.  A launch sequence that ended in a refusal after its first kernels (a backward with a misaligned
dk stride) is recorded as the refusal.  No DD_* variable was set.  Re-record only when a decision is changed on purpose, and say which.

The file holds `outcomes` (the distinct outcome rows, int32 [k, OUT_N], attention_plan_cases.OUT_FIELDS), `index` (uint16 [n]: the outcome
of every case, in generator order), `block_names` / `block_sizes`, and `cases_sha256` (hash of the generated case list).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import attention_plan_cases as cases  # noqa: E402


def save(res, blks, path=os.path.join(HERE, "attention_plan_table.npz")):
    outcomes, index = np.unique(res, axis=0, return_inverse=True)
    assert len(outcomes) < 65536
    np.savez_compressed(path, outcomes=outcomes.astype(np.int32), index=index.reshape(-1).astype(np.uint16),
                        block_names=np.array([n for n, _r in blks]), block_sizes=np.array([len(r) for _n, r in blks], dtype=np.int64),
                        cases_sha256=np.array(cases.cases_hash(blks)))
    print("%d cases, %d outcomes, %d bytes -> %s" % (len(res), len(outcomes), os.path.getsize(path), path))
    routes, counts = np.unique(res[:, 0], return_counts=True)
    print("cases per route:", dict(zip(routes.tolist(), counts.tolist())))


def main():
    from distdiff_amd import _lib
    _lib.lib()
    blks = list(cases.blocks())
    save(np.concatenate([cases.evaluate(_lib.LIB_PATH, rows) for _name, rows in blks]), blks)


if __name__ == "__main__":
    main()
