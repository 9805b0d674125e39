"""Interleaved A/B of builds of libsfmhip.so on the C3 exact-float match step (257 x 4096 x
256-d, int16 graph: the call dist.match_all_pairs_sharded makes), in one process on one device:

    python tools/bench_match_valueonly_ab.py [--rounds N] [--entry NAME] [--other-entry NAME] [--d D] OTHER_LIB.so [...]

The other libraries (e.g. the parent commit's build under another file name) and the tree's
library all run on the same bank (quantised operands, keys and residual bounds of the tree's
library), one call each per round in turn, on the full pair list and on the pairs with |a - b| <= 2
(the overlapping images, where the certificate accepts ~15 % of the rows).  Prints per arm the
median / min / max step time over the rounds, rows_rescored and a checksum of the match graph.
--entry sfmhip_match_pairs_exact_fp6_i16 runs the tree's arm through the FP6 entry (the bank's grid
values, codes and their norms, keys and bounds: DESIGN.md K1''); the other libraries keep
sfmhip_match_pairs_exact_i16 on the int8 operands, so a parent build without the entry can be the
other arm, unless --other-entry sfmhip_match_pairs_exact_fp6_i16 sends them through their FP6 entry
too.  An FP6 arm gets the operand array its library reads: the dense rows (bank.dense) when the library
exports sfmhip_desc_pack_fp6, the 32-byte chunks of the quantiser (bank.code) when it does not — a
parent build from before the dense layout.  --d 128 runs the step on 257 x 4096 x 128-d descriptors."""
import ctypes
import hashlib
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfm = importlib.import_module("3d_reconstruction_amd")
abi = importlib.import_module("3d_reconstruction_amd._abi")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")

args = sys.argv[1:]
rounds = 12
if args and args[0] == "--rounds":
    rounds, args = int(args[1]), args[2:]
NAME = "sfmhip_match_pairs_exact_i16"
TREE_NAME = NAME
if args and args[0] == "--entry":
    TREE_NAME, args = args[1], args[2:]
OTHER_NAME = NAME
if args and args[0] == "--other-entry":
    OTHER_NAME, args = args[1], args[2:]
D = 256
if args and args[0] == "--d":
    D, args = int(args[1]), args[2:]
FP6_NAME = "sfmhip_match_pairs_exact_fp6_i16"
if TREE_NAME not in (NAME, FP6_NAME) or OTHER_NAME not in (NAME, FP6_NAME):
    raise SystemExit(f"--entry and --other-entry must be {NAME} or {FP6_NAME}")
arms = []
for path in args:
    lib = ctypes.CDLL(os.path.abspath(path))
    getattr(lib, OTHER_NAME).argtypes = abi.SIGNATURES[OTHER_NAME]
    getattr(lib, OTHER_NAME).restype = ctypes.c_int
    arms.append((os.path.basename(path), lib))
arms.append(("tree", abi.lib))

dev = torch.device("cuda", 0)
x = syn.superpoint_like(257, 4096, D, seed=1, device=dev)
bank = sfm.DescriptorBank.from_float(x, mode=sfm.MODE_FLOAT)
del x
allp = sfm.all_pairs(257)
near = allp[(allp[:, 1] - allp[:, 0]) <= 2]
ptr, sp = abi.ptr, abi.stream_ptr
print(f"device {torch.cuda.get_device_name(0)}, rounds {rounds}, d {D}", flush=True)
for label, pairs in (("full", allp), ("near", near)):
    pr = abi.dev(pairs, torch.int32)
    P = int(pr.shape[0])
    outs = {n: torch.empty((P, bank.m_pad), dtype=torch.int16, device=dev) for n, _ in arms}
    nres = torch.zeros(1, dtype=torch.int32, device=dev)

    def step(lib, out):
        if (TREE_NAME if lib is abi.lib else OTHER_NAME) == FP6_NAME:
            operands = bank.dense if hasattr(lib, "sfmhip_desc_pack_fp6") else bank.code
            rc = getattr(lib, FP6_NAME)(ptr(operands), ptr(bank.g), ptr(bank.gnorms), ptr(bank.gkeys), ptr(bank.x),
                                        ptr(bank.gerow), ptr(bank.geimg), ptr(bank.n_kpts), bank.n_img, bank.m_pad,
                                        bank.d, ptr(pr), P, 3, 4, ptr(out), ptr(nres), sp())
            if rc:
                raise RuntimeError(f"{FP6_NAME} failed: {rc}")
            return
        rc = getattr(lib, NAME)(ptr(bank.qm), ptr(bank.norms), ptr(bank.keys), ptr(bank.q), ptr(bank.x),
                                ptr(bank.erow), ptr(bank.eimg), bank.mode, ptr(bank.n_kpts), bank.n_img, bank.m_pad,
                                bank.d, ptr(pr), P, 3, 4, ptr(out), ptr(nres), sp())
        if rc:
            raise RuntimeError(f"{NAME} failed: {rc}")

    ts = {n: [] for n, _ in arms}
    res = {}
    for n, lib in arms:   # warm-up, one call each
        step(lib, outs[n])
        torch.cuda.synchronize()
        res[n] = int(nres.item())
    for _ in range(rounds):
        for n, lib in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(lib, outs[n])
            e1.record()
            torch.cuda.synchronize()
            ts[n].append(e0.elapsed_time(e1))
    for n, _ in arms:
        t = np.array(ts[n])
        h = hashlib.sha256(outs[n].cpu().numpy().tobytes()).hexdigest()[:16]
        print(f"{label} ({P} pairs) {n}: median {np.median(t):.3f} ms  min {t.min():.3f}  max {t.max():.3f}  "
              f"rows_rescored {res[n]}  graph sha {h}", flush=True)
        print(f"    rounds in order: {' '.join(f'{v:.3f}' for v in t)}", flush=True)
    del outs
    torch.cuda.empty_cache()
