"""Paired comparison of two validations that carry the same bootstrap: ``python compare_runs.py a=<bootstrap_<task>.pt>
b=<bootstrap_<task>.pt>``.

Two runs validated with the same ``bootstrap.seed`` and replicate count on the same split give every sample the same weight in
replicate r, so replicate r of run b minus replicate r of run a is one draw of the DIFFERENCE under the sampling noise of the split
-- the two runs' noise is not added, it cancels where they agree.  The pair is refused unless seed, replicates and split agree and
the row-count column of every shared group -- ``acc_den[:, 0]``, the sum of the weights per replicate, which does not depend on the
model -- is equal bit for bit: the same samples under the same weights.

Per shared metric: the difference of the point estimates, the [lo, hi] of b_r - a_r by the interval rule of the meters
(``meters.bootstrap_interval``) and p = (1 + #{r : b_r - a_r <= 0}) / (R + 1), the one-sided achieved significance of "b is not
above a".  No GPU: the files hold CPU tensors."""
from __future__ import annotations

import sys
from typing import Dict

import torch

from .meters import bootstrap_interval


def check_pair(a: dict, b: dict) -> None:
    """A ValueError that names what differs: seed, replicates, split, or the valid counts of a shared group."""
    for field in ("seed", "replicates", "split"):
        if a.get(field) != b.get(field):
            raise ValueError(f"compare_runs: the two files differ in {field} ({a.get(field)!r} / {b.get(field)!r}): their replicates are not paired")
    shared = [g for g in a["groups"] if g in b["groups"]]
    if not shared:
        raise ValueError(f"compare_runs: the two files share no group of metrics ({sorted(a['groups'])} / {sorted(b['groups'])})")
    for g in shared:
        na, nb = a["groups"][g]["acc_den"][:, 0], b["groups"][g]["acc_den"][:, 0]
        if na.shape != nb.shape or not torch.equal(na, nb):
            bad = int((na != nb).sum()) if na.shape == nb.shape else -1
            raise ValueError(f"compare_runs: the valid counts of group '{g}' differ in {bad} of {a['replicates']} replicates: the two runs did "
                             "not see the same samples under the same weights")


def compare(a: dict, b: dict) -> Dict[str, dict]:
    """metric -> {"a", "b", "diff", "lo", "hi", "se", "p", "valid"} for every metric both files hold (``check_pair`` first)."""
    check_pair(a, b)
    R, level, out = int(a["replicates"]), float(a["level"]), {}
    for k, va in a["values"].items():
        if k not in b["values"]:
            continue
        d = b["values"][k].double() - va.double()  # (NaN where either run dropped the replicate)
        ci = bootstrap_interval(d, level, R)
        ok = d[~torch.isnan(d)]
        pa, pb = a["point"].get(k), b["point"].get(k)
        out[k] = {"a": pa, "b": pb, "diff": None if pa is None or pb is None else pb - pa,
                  "lo": None if ci is None else ci["lo"], "hi": None if ci is None else ci["hi"], "se": None if ci is None else ci["se"],
                  "p": (1 + int((ok <= 0).sum())) / (R + 1), "valid": int(ok.numel())}
    return out


def lines(res: Dict[str, dict], level: float) -> list:
    out = []
    for k, r in res.items():
        ci = "no interval (fewer than half of the replicates valid)" if r["lo"] is None else f"{level * 100:g}% [{r['lo']:+.6f}, {r['hi']:+.6f}]"
        diff = "n/a" if r["diff"] is None else f"{r['diff']:+.6f}"
        out.append(f"{k}: b - a = {diff}  {ci}  p(b <= a) = {r['p']:.4f}  ({r['valid']} replicates)")
    return out


def main(argv=None) -> Dict[str, dict]:
    argv = sys.argv[1:] if argv is None else list(argv)
    args = dict(x.split("=", 1) for x in argv if "=" in x)
    if set(args) != {"a", "b"} or len(args) != len(argv):
        raise SystemExit("usage: python compare_runs.py a=<bootstrap_<task>.pt> b=<bootstrap_<task>.pt>")
    a, b = (torch.load(args[k], map_location="cpu", weights_only=False) for k in ("a", "b"))
    res = compare(a, b)
    print(f"a = {args['a']}\nb = {args['b']}\nseed {a['seed']}, {a['replicates']} replicates, split {a['split']}, {a['clusters']} clusters")
    for line in lines(res, float(a["level"])):
        print(line)
    return res


if __name__ == "__main__":
    main()
