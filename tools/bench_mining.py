"""Time one triplet-mining round (kp2d_vpr_mine) and one get_positives against the host path they replace.

    python3 tools/bench_mining.py [--numDb 10000] [--numQ 7000] [--dim 4096] [--host-queries 500]
                                  [--out profiles/triplet_mining.json] [--commit NAME]

Inputs: synthetic.vpr_struct + synthetic.place_descriptors (no dataset ships here), the reference's defaults otherwise
(nNegSample 1000, nNeg 10, nNegFactor 10, margin 0.1).
Device: TripletMiner.mine on device tensors, the database pack included (the features are new after every cache refresh);
HIP-event time per round, the best of three windows of back-to-back rounds after a warm-up round.  get_positives: wall
clock from numpy positions to the array of index arrays.
Host baseline: the features as numpy, then the reference's steps per query (src/data/pittsburgh.py:303-333: two
sklearn NearestNeighbors fits, np.random.choice, np.unique), wall clock over the first --host-queries queries that have a
positive, scaled to all of them (both figures are recorded); NearestNeighbors.radius_neighbors for get_positives.
Nothing is gated on the result; the file is where the numbers go.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_round(feat, numDb, queries, nontrivial_positives, potential_negatives, nNegSample, nNeg, nNegFactor, margin):
    """The reference's __getitem__ (features from an array) for the given queries -> number of triplets."""
    from sklearn.neighbors import NearestNeighbors
    negCache = [np.empty((0,)) for _ in range(len(nontrivial_positives))]
    found = 0
    for index in queries:
        qFeat = feat[index + numDb]
        posFeat = feat[nontrivial_positives[index].tolist()]
        knn = NearestNeighbors(n_jobs=1)
        knn.fit(posFeat)
        dPos, posNN = knn.kneighbors(qFeat.reshape(1, -1), 1)
        dPos = dPos.item()
        negSample = np.random.choice(potential_negatives[index], nNegSample)
        negSample = np.unique(np.concatenate([negCache[index], negSample]))
        negFeat = feat[list(map(int, negSample))]
        knn.fit(negFeat)
        dNeg, negNN = knn.kneighbors(qFeat.reshape(1, -1), min(nNeg * nNegFactor, len(negSample)))
        violatingNeg = dNeg.reshape(-1) < dPos + margin ** 0.5
        if np.sum(violatingNeg) < 1:
            continue
        negCache[index] = negSample[negNN.reshape(-1)[violatingNeg][:nNeg]].astype(np.int32)
        found += 1
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numDb", type=int, default=10000)
    ap.add_argument("--numQ", type=int, default=7000)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--host-queries", type=int, default=500)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--commit", default="", help="recorded when the tree is not a git checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triplet_mining.json"))
    args = ap.parse_args()
    import torch
    from sklearn.neighbors import NearestNeighbors
    from nano_vs_slam_amd import mining, synthetic

    st = synthetic.vpr_struct(args.numDb, args.numQ, 1)
    dbFeat = synthetic.place_descriptors(st.utmDb, args.dim, 4, noise_seed=0)
    qFeat = synthetic.place_descriptors(st.utmQ, args.dim, 4, noise_seed=1)
    res = {"device": torch.cuda.get_device_name(0), "numDb": args.numDb, "numQ": args.numQ, "dim": args.dim, "nNegSample": 1000,
           "nNeg": 10, "nNegFactor": 10, "margin": 0.1,
           "commit": subprocess.run(["git", "describe", "--always", "--dirty"], cwd=ROOT, capture_output=True,
                                    text=True).stdout.strip() or args.commit or "unknown"}

    # get_positives
    mining.get_positives(st.utmDb, st.utmQ, st.posDistThr)                  # warm-up (library load, allocator)
    t = time.perf_counter()
    gt = mining.get_positives(st.utmDb, st.utmQ, st.posDistThr)
    res["get_positives_ms"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    knn = NearestNeighbors(n_jobs=1)
    knn.fit(st.utmDb)
    ref = knn.radius_neighbors(st.utmQ, radius=st.posDistThr, return_distance=False)
    res["get_positives_sklearn_ms"] = (time.perf_counter() - t) * 1e3
    assert all(np.array_equal(a, np.sort(b)) for a, b in zip(gt, ref))

    # one mining round on the device
    db_t, q_t = torch.from_numpy(dbFeat).cuda(), torch.from_numpy(qFeat).cuda()
    for prec in ("f16x3", "fp32"):
        miner = mining.TripletMiner(st.utmDb, st.utmQ, st.posDistThr, st.nonTrivPosDistSqThr, precision=prec)
        out = miner.mine(db_t, q_t)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); miner.mine(db_t, q_t); e.record(); torch.cuda.synchronize()
        reps = max(1, int(args.window * 1000 / max(s.elapsed_time(e), 1e-3)))
        best = None
        for _ in range(3):
            s.record()
            for _ in range(reps):
                miner.mine(db_t, q_t)
            e.record()
            torch.cuda.synchronize()
            ms = s.elapsed_time(e) / reps
            best = ms if best is None else min(best, ms)
        res[f"mine_round_{prec}_ms"] = best
        res[f"triplets_{prec}"] = int((out[2] > 0).sum())
    res["queries_with_positive"] = int(len(miner.queries))

    # the host path
    feat = np.concatenate([dbFeat, qFeat])
    ntp, potneg = miner.nontrivial_positives, miner.potential_negatives
    sub = miner.queries[:args.host_queries]
    np.random.seed(0)
    t = time.perf_counter()
    found = host_round(feat, args.numDb, sub, ntp, potneg, 1000, 10, 10, 0.1)
    host_ms = (time.perf_counter() - t) * 1e3
    res.update(host_queries_timed=int(len(sub)), host_triplets=found, host_sklearn_ms_timed=host_ms,
               host_sklearn_ms_scaled_to_all=host_ms * len(miner.queries) / max(len(sub), 1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
