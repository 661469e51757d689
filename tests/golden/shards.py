"""Store a (nested) dict of tensors as several small files.

A golden dict is flattened to (key path, leaf) pairs, packed in order into
shards of at most SHARD_BYTES of tensor data, and written as
`<stem>.000.pt`, `<stem>.001.pt`, ...; load_sharded() puts the same dict back
together (same keys, same order, same values). Keeps every committed fixture
file well under 1 MiB."""

import glob
import os

import torch

SHARD_BYTES = 768 * 1024


def _flatten(obj, path, out):
    if isinstance(obj, dict) and obj and all(isinstance(k, str) for k in obj):
        for k, v in obj.items():
            _flatten(v, path + (k,), out)
    else:
        out.append((path, obj))


def _nbytes(leaf):
    return leaf.numel() * leaf.element_size() if torch.is_tensor(leaf) else 64


def save_sharded(obj, stem):
    for old in glob.glob(glob.escape(stem) + ".[0-9][0-9][0-9].pt"):
        os.remove(old)
    leaves = []
    _flatten(obj, (), leaves)
    shards, cur, cur_bytes = [], [], 0
    for path, leaf in leaves:
        n = _nbytes(leaf)
        if cur and cur_bytes + n > SHARD_BYTES:
            shards.append(cur)
            cur, cur_bytes = [], 0
        # clone: a view would drag its whole storage into the shard
        cur.append((path, leaf.clone() if torch.is_tensor(leaf) else leaf))
        cur_bytes += n
    if cur:
        shards.append(cur)
    paths = []
    for i, shard in enumerate(shards):
        paths.append(f"{stem}.{i:03d}.pt")
        torch.save(shard, paths[-1])
    return paths


def load_sharded(stem):
    paths = sorted(glob.glob(glob.escape(stem) + ".[0-9][0-9][0-9].pt"))
    if not paths:
        raise FileNotFoundError(f"no shards for {stem}")
    out = {}
    for p in paths:
        for path, leaf in torch.load(p, weights_only=False):
            d = out
            for k in path[:-1]:
                d = d.setdefault(k, {})
            d[path[-1]] = leaf
    return out
