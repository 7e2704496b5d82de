"""Host model of the cluster bootstrap (include/egopack_bootstrap.h), in numpy over tests/philox_ref.py: the
Poisson(1) weights, the integer accumulators, the replicate values and the interval rule.  Independent of the package (nothing is
imported from ``egopack_amd``): integer arithmetic up to the replicate values, which are float64 quotients of the same integers, so
every comparison of accumulators is ``torch.equal`` / ``numpy.array_equal``."""
import math
from decimal import Decimal, getcontext

import numpy as np

from tests import philox_ref as PR

# T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!), k = 0 .. 11 (the header's table; ``table()`` recomputes it)
T = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463, 4294966817,
     4294967252, 4294967292)
KEY_SALT = 0x424F4F545F434C55  # "BOOT_CLU" (ops.BOOTSTRAP_KEY_SALT)
MAX_R, MAX_M, MAX_C, MAX_CLUSTER = 65536, 8, 1024, (1 << 40) - 1


def table(n=12, digits=60):
    """The table in ``digits``-digit decimals."""
    getcontext().prec = digits
    e_inv = 1 / Decimal(1).exp()
    out, cdf, fact = [], Decimal(0), Decimal(1)
    for k in range(n):
        if k:
            fact *= k
        cdf += e_inv / fact
        out.append(int((cdf * (1 << 32)).to_integral_value(rounding="ROUND_FLOOR")))
    return tuple(out)


def key(seed):
    return (int(seed) ^ KEY_SALT) & PR.MASK64


def words(cluster, R, k):
    """uint32 [rows, R]: the Philox word of (cluster, replicate) -- word r & 3 of counter (c << 14) | (r >> 2); clusters >= 0."""
    c = np.asarray(cluster, dtype=np.int64).astype(np.uint64)
    groups = (int(R) + 3) // 4
    ctr = (c[:, None] << np.uint64(14)) | np.arange(groups, dtype=np.uint64)[None, :]
    return PR.philox_u64(ctr, k).reshape(c.shape[0], groups * 4)[:, :int(R)]


def weights(cluster, R, k):
    """uint8 [rows, R]: w = #{j : word >= T[j]}; 0 for a negative cluster id."""
    cluster = np.asarray(cluster, dtype=np.int64)
    ok = cluster >= 0
    w = np.zeros((cluster.shape[0], int(R)), dtype=np.uint8)
    if ok.any():
        wd = words(cluster[ok], R, k).astype(np.uint64)
        w[ok] = sum((wd >= np.uint64(t)).astype(np.uint8) for t in T)
    return w


def empty(R, M, C=0):
    acc = {"acc_num": np.zeros((R, M), dtype=np.int64), "acc_den": np.zeros((R, M), dtype=np.int64)}
    if C:
        acc.update(cls_num=np.zeros((R, C), dtype=np.int64), cls_den=np.zeros((R, C), dtype=np.int64))
    return acc


def accumulate(acc, cluster, num, den, k, label=None, class_col=-1):
    """Adds one launch to ``acc`` (``empty``'s dict), in int64 (sums wrap as on the device)."""
    num, den = np.asarray(num, dtype=np.int64), np.asarray(den, dtype=np.int64)
    R = acc["acc_num"].shape[0]
    w = weights(cluster, R, k).astype(np.int64)  # [rows, R]
    with np.errstate(over="ignore"):
        acc["acc_num"] += w.T @ num
        acc["acc_den"] += w.T @ den
    if class_col >= 0:
        C = acc["cls_num"].shape[1]
        y = np.asarray(label, dtype=np.int64)
        inside = (y >= 0) & (y < C)
        for name, src in (("cls_num", num), ("cls_den", den)):
            rows = inside & (src[:, class_col] != 0)
            t = np.zeros((C, R), dtype=np.int64)
            np.add.at(t, y[rows], w[rows])
            acc[name] += t.T
    return acc


def ratio_values(acc_num, acc_den):
    """float64 [R]: num / den per replicate, NaN where den == 0."""
    num, den = np.asarray(acc_num, dtype=np.int64), np.asarray(acc_den, dtype=np.int64)
    out = np.full(num.shape, np.nan, dtype=np.float64)
    ok = den != 0
    out[ok] = num[ok].astype(np.float64) / den[ok].astype(np.float64)
    return out


def mean_class_values(cls_num, cls_den):
    """float64 [R]: the mean over the classes with cls_den > 0 of cls_num / cls_den, NaN for a replicate without a class."""
    num, den = np.asarray(cls_num, dtype=np.int64), np.asarray(cls_den, dtype=np.int64)
    out = np.full(num.shape[0], np.nan, dtype=np.float64)
    for r in range(num.shape[0]):
        seen = den[r] > 0
        if seen.any():
            out[r] = float(np.sum(num[r][seen].astype(np.float64) / den[r][seen].astype(np.float64))) / int(seen.sum())
    return out


def interval(values, level, R):
    """{"lo", "hi", "se", "valid", "dropped"} or None (fewer than R / 2 valid): v sorted, j = floor((1 - level) / 2 * n), lo = v[j],
    hi = v[n - 1 - j], se = the standard deviation with divisor n - 1.  (1e-9 before the floor: 0.05 / 2 * 1000 is 25 in decimal.)"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    total = v.size
    v = np.sort(v[~np.isnan(v)])
    n = v.size
    if n == 0 or 2 * n < R:
        return None
    j = int(math.floor((1.0 - level) / 2.0 * n + 1e-9))
    return {"lo": float(v[j]), "hi": float(v[n - 1 - j]), "se": float(np.std(v, ddof=1)) if n > 1 else 0.0, "valid": n, "dropped": total - n}


def tables(groups, seed, R, level=0.95, split="val", clusters=0, point=None):
    """A file as ``train.save_bootstraps`` writes it, from model accumulators: ``groups`` = {name: (keys, class_key, acc dict)}."""
    import torch
    out = {"seed": seed, "replicates": R, "level": level, "split": split, "clusters": clusters, "groups": {}, "values": {}, "point": {}}
    for name, (keys, class_key, acc) in groups.items():
        out["groups"][name] = {"keys": list(keys), "class_key": class_key, **{k: torch.from_numpy(v.copy()) for k, v in acc.items()}}
        for m, k in enumerate(keys):
            if k is not None:
                out["values"][k] = torch.from_numpy(ratio_values(acc["acc_num"][:, m], acc["acc_den"][:, m]))
        if class_key is not None:
            out["values"][class_key] = torch.from_numpy(mean_class_values(acc["cls_num"], acc["cls_den"]))
    out["point"] = dict(point or {})
    return out
