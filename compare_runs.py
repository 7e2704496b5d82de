#!/usr/bin/env python3
"""The interval of the DIFFERENCE between two validations that carry the same bootstrap (bootstrap.replicates > 0, one seed):

    python compare_runs.py a=<run a>/bootstrap_ar.pt b=<run b>/bootstrap_ar.pt

Per shared metric: b - a of the point estimates, the [lo, hi] of the replicate differences and p(b <= a).  Refused unless seed,
replicates, split and the per-replicate valid counts agree.  No GPU.  The logic lives in egopack_amd.compare."""
from egopack_amd.compare import compare, main  # noqa: F401

if __name__ == "__main__":
    main()
