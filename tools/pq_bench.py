"""PQIndex (dsub 8 and 16) against SQ8Index and the f32 FAISSIndex on the same vectors in the same run (HIP events, mean
of --reps after --warmup).

1 M x 128 random unit rows (the incompressible worst case for a product quantiser).  Serve leg: IVF 100/10, batch 256,
k = 500.  Flat leg: a one-list index, 4 096 queries, k = 500.  Per leg: search time of every index (the quantised ones in
their automatic mode and with each emission forced), the PQ build time split into range pass + SQ8 encode, training per
Lloyd step and final assignment, device bytes held and at the build's peak, recall@10 and recall@500 against the f32
lists, plain and refined at factors 2 / 4 / 8 with the certified share.

Gather leg: what the data-dependent LDS gathers of the PQ scan cost.  The same one-list scan (dense emission, 256 queries)
over a corpus of identical rows -- every row names entry 0, so every gather of a wave reads one address per sub-space: a
broadcast, no bank conflict -- against the scan over the random rows.  The results of that index are meaningless; only the
time is of interest, and of it only the scan kernel's: the select behind it is slower on all-equal scores, so compare the
kernel times of a kernel trace of one run per corpus (--gather-corpus random / same), not the whole-search times.

Embeddings leg: recall on the item embeddings of a short ml1m_like() training run (3 883 items, d = 64, exact index,
queries = the user embeddings).  Recall is from one run and unpinned.

Residual legs (by_residual=True, the codebooks quantise the rows' codes minus their list's centroid code): every leg over
an IVF index also builds and searches the residual PQ index of each dsub next to the plain one, in the same run, under
the keys pqr8_ / pqr16_ (the kernel that fills T, sq8_pair_offset_kernel, is read from a kernel trace of such a run: HIP
events around a whole search cannot separate it).  serve4096 is
the serve leg at 4 096 queries; clustered is the serve leg over a clustered corpus (--n unit rows around 100 centres,
lists trained on it); the embeddings leg adds an IVF index of the same embeddings (16 lists, all probed, so recall
measures the codes and not the probing) with the plain and the residual PQ index over it.  --no-residual leaves the
residual legs out (the plain legs then run exactly as before).

python tools/pq_bench.py [--legs serve,serve4096,clustered,flat,gather,embeddings] [--reps 20] [--warmup 3] [--n 1000000]
                         [--iters 10] [--no-residual]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from recommendit_amd import FAISSIndex, PQIndex, SQ8Index  # noqa: E402

K = 500
ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="serve,flat,gather,embeddings")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--epochs", type=int, default=2)
ap.add_argument("--modes", default="auto,dense,thresholded")
ap.add_argument("--no-residual", action="store_true", help="leave the by_residual legs out")
ap.add_argument("--spread", type=float, default=0.25, help="clustered corpus: noise around a centre, relative to its norm")
ap.add_argument("--gather-corpus", default="both", choices=["both", "random", "same"],
                help="gather leg: one corpus only, so that a kernel trace of the run holds one kind of scan")
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
g = torch.Generator(device=dev)
g.manual_seed(7)
out = {}


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps


def unit(n, d):
    x = torch.randn((n, d), device=dev, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def recall(ref: torch.Tensor, got: torch.Tensor, k: int) -> float:
    """mean share of the reference's first k ids found among the first k ids returned"""
    r, x = ref[:, :k], got[:, :k]
    hit = (r.unsqueeze(2) == x.unsqueeze(1)).any(dim=2) & (r >= 0)
    return float(hit.sum().item()) / max(1, int((r >= 0).sum().item()))


def show(tag, row):
    print(f"[pq] {tag}: " + ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()), flush=True)


def quality(idx, q, ref, k, row, pre):
    _, got = idx.batch_search_device(q, k=k, normalized=True)
    row[f"{pre}recall@10"] = recall(ref, got, 10)
    row[f"{pre}recall@{k}"] = recall(ref, got, k)
    if idx.has_vectors:
        for f in (2, 4, 8):
            _, got, cert, _ = idx.batch_search_device(q, k=k, normalized=True, refine=f, return_cert=True)
            row[f"{pre}refine{f}_recall@10"] = recall(ref, got, 10)
            row[f"{pre}refine{f}_recall@{k}"] = recall(ref, got, k)
            row[f"{pre}refine{f}_certified"] = float(cert.float().mean().item())


def build_pq(f32, dsub, row, pre, keep=True, by_residual=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pq = PQIndex.from_index(f32, dsub=dsub, n_iter=args.iters, keep_vectors=False, by_residual=by_residual)
    torch.cuda.synchronize()
    row[f"{pre}build_ms"] = (time.perf_counter() - t0) * 1e3
    ts, st = pq.train_stats(), pq.stats()
    row[f"{pre}range_encode_ms"] = ts["range_encode_ms"]
    row[f"{pre}train_ms_per_iter"] = ts["train_ms"] / max(1, args.iters)
    row[f"{pre}assign_ms"] = ts["assign_ms"]
    row[f"{pre}device_bytes"] = st["device_bytes"]
    row[f"{pre}peak_build_bytes"] = ts["peak_bytes"]
    row[f"{pre}bytes_per_vector"] = st["bytes_per_vector"]
    row[f"{pre}distortion_first_last"] = [int(ts["distortion"][0]), int(ts["distortion"][-1])]
    if by_residual:
        row[f"{pre}residual_clamped"] = ts["residual_clamped"]
    if keep:
        pq.attach_vectors(f32)
    return pq


def leg(name, f32, nq, d, queries=None):
    q = unit(nq, d)
    if queries is not None:   # around the given points instead of uniform on the sphere
        q = queries(nq) + (args.spread / d ** 0.5) * torch.randn((nq, d), device=dev, generator=g)
        q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    k = min(K, f32.index.ntotal)
    row = {"f32_ms": timed(lambda: f32.batch_search_device(q, k=k, normalized=True))}
    _, ref = f32.batch_search_device(q, k=k, normalized=True)
    sq = SQ8Index.from_index(f32, keep_vectors=True)
    row["sq8_device_bytes"] = sq.stats()["device_bytes"]
    row["sq8_auto_ms"] = timed(lambda: sq.batch_search_device(q, k=k, normalized=True))
    quality(sq, q, ref, k, row, "sq8_")
    sq.drop_vectors()
    del sq
    residual = bool(f32.index.is_ivf) and not args.no_residual
    for dsub, by_res in [(d_, r_) for d_ in (8, 16) for r_ in ((False, True) if residual else (False,))]:
        pre = f"pqr{dsub}_" if by_res else f"pq{dsub}_"
        pq = build_pq(f32, dsub, row, pre, by_residual=by_res)
        for mode in filter(None, args.modes.split(",")):
            n0, r0 = pq.search_stats()
            row[f"{pre}{mode}_ms"] = timed(lambda: pq.batch_search_device(q, k=k, normalized=True, mode=mode))
            n1, r1 = pq.search_stats()
            row[f"{pre}{mode}_redone_share"] = (r1 - r0) / max(1, n1 - n0)
        quality(pq, q, ref, k, row, pre)
        del pq
        torch.cuda.empty_cache()
    out[name] = row
    show(name, row)


def gather_leg():
    """dense one-list scan at 256 queries: random rows (gathers spread over the codebooks) against identical rows (every
    gather a broadcast of entry 0)"""
    nq, d = 256, 128
    q = unit(nq, d)
    row = {}
    which = args.gather_corpus
    if which in ("both", "random"):
        rnd = FAISSIndex(embed_dim=d, exact=True)
        rnd.build_from_device(unit(args.n, d), np.arange(1, args.n + 1))
        if which == "both":
            sq = SQ8Index.from_index(rnd)
            row["sq8_dense_ms"] = timed(lambda: sq.batch_search_device(q, k=K, normalized=True, mode="dense"))
            del sq
        for dsub in (8, 16):
            a = PQIndex.from_index(rnd, dsub=dsub, n_iter=1)
            row[f"pq{dsub}_dense_ms"] = timed(lambda: a.batch_search_device(q, k=K, normalized=True, mode="dense"))
            del a
        del rnd
    if which in ("both", "same"):
        same = FAISSIndex(embed_dim=d, exact=True)
        same.build_from_device(unit(1, d).expand(args.n, d).contiguous(), np.arange(1, args.n + 1))
        for dsub in (8, 16):
            b = PQIndex.from_index(same, dsub=dsub, n_iter=0)
            assert int(b.pq_codes().max()) == 0
            row[f"pq{dsub}_dense_fixed_entry_ms"] = timed(lambda: b.batch_search_device(q, k=K, normalized=True, mode="dense"))
            del b
    out["gather nq=256 dense"] = row
    show("gather nq=256 dense", row)


def embeddings_leg():
    from recommendit_amd import synthetic as GB
    from recommendit_amd.train_embeddings import EmbeddingTrainer, build_item_genre_dict
    ratings, movies, _ = GB.ml1m_like()
    item_ids = np.asarray(sorted(movies["item_id"].unique().tolist()), dtype=np.int64)
    gd = build_item_genre_dict(movies)
    with tempfile.TemporaryDirectory() as td:
        tr = EmbeddingTrainer(model_output_path=os.path.join(td, "m.pt"), epochs=args.epochs, seed=0)
        model = tr.train(ratings, movies)
    E = model.get_item_embeddings(item_ids.tolist(), np.stack([gd[i] for i in item_ids.tolist()]))
    users = np.unique(ratings["user_id"].to_numpy())[:4096]
    q = model.get_user_embeddings(users.tolist(), as_tensor=True)
    q = (q / q.norm(dim=1, keepdim=True).clamp(min=1e-8)).contiguous()
    f32 = FAISSIndex(embed_dim=E.shape[1], exact=True)
    f32.build_ivf_index(E, item_ids.tolist())
    k = min(K, len(item_ids))
    _, ref = f32.batch_search_device(q, k=k, normalized=True)
    row = {"items": int(len(item_ids)), "d": int(E.shape[1]), "queries": int(q.shape[0]), "epochs": args.epochs}
    sq = SQ8Index.from_index(f32, keep_vectors=True)
    quality(sq, q, ref, k, row, "sq8_")
    for dsub in (8, 16):
        pq = build_pq(f32, dsub, {}, "")
        quality(pq, q, ref, k, row, f"pq{dsub}_")
    if not args.no_residual:
        ivf = FAISSIndex(embed_dim=E.shape[1], n_lists=16, n_probe=16)
        ivf.build_ivf_index(E, item_ids.tolist())
        _, ref_ivf = ivf.batch_search_device(q, k=k, normalized=True)
        row["ivf16_f32_recall@10_of_exact"] = recall(ref, ref_ivf, 10)
        for dsub in (8, 16):
            for by_res in (False, True):
                pq = build_pq(ivf, dsub, {}, "", by_residual=by_res)
                quality(pq, q, ref, k, row, f"ivf16_pq{'r' if by_res else ''}{dsub}_")
    out["ml1m_like item embeddings"] = row
    show("ml1m_like item embeddings", row)


for which in filter(None, args.legs.split(",")):
    if which == "serve":
        idx = FAISSIndex(embed_dim=128, n_lists=100, n_probe=10)
        idx.build_from_device(unit(args.n, 128), np.arange(1, args.n + 1))
        leg("serve ivf100/10 nq=256", idx, 256, 128)
        del idx
    elif which == "serve4096":
        idx = FAISSIndex(embed_dim=128, n_lists=100, n_probe=10)
        idx.build_from_device(unit(args.n, 128), np.arange(1, args.n + 1))
        leg("serve ivf100/10 nq=4096", idx, 4096, 128)
        del idx
    elif which == "clustered":
        cen = unit(100, 128)
        x = cen[torch.randint(0, 100, (args.n,), device=dev, generator=g)] + (args.spread / 128 ** 0.5) * torch.randn(
            (args.n, 128), device=dev, generator=g)
        x = (x / x.norm(dim=1, keepdim=True)).contiguous()
        idx = FAISSIndex(embed_dim=128, n_lists=100, n_probe=10)
        idx.build_from_device(x, np.arange(1, args.n + 1))
        # queries: corpus-like points (fresh noise around the same centres)
        for nq in (256, 4096):
            leg(f"clustered ivf100/10 nq={nq}", idx, nq, 128, queries=lambda n: cen[torch.randint(0, 100, (n,), device=dev, generator=g)])
        del idx, x
    elif which == "flat":
        idx = FAISSIndex(embed_dim=128, exact=True)
        idx.build_from_device(unit(args.n, 128), np.arange(1, args.n + 1))
        leg("one list nq=4096", idx, 4096, 128)
        del idx
    elif which == "gather":
        gather_leg()
    elif which == "embeddings":
        embeddings_leg()
    else:
        raise SystemExit(f"unknown leg {which!r}")
    torch.cuda.empty_cache()
print(json.dumps(out))
