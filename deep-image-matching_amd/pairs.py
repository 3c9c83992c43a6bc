"""Pair generation on the device: ``matching_lowres`` (the reference's default CLI strategy).

Restatement of ``pairs_generator.py``: ``pairs_from_sequential`` (:22-34), ``pairs_from_bruteforce``
(:37-38) and the SuperPoint branch of ``pairs_from_lowres`` (:41-235, the only branch that runs —
``use_superpoint = True`` is hard-wired at :95): every image is read as grey, down-sampled with
``cv2.resize(..., INTER_AREA)`` to ``resize_max`` on its long side, described by hloc's SuperPoint wrapper
(nms 3 / 2048 keypoints / threshold 0.0005 + the wrapper's ``fix_sampling=True``, Q3) and every image pair
is matched with LightGlue (7 layers, depth 0.9 / width 0.95 / filter 0.3, no ``image_size``: keypoint
extent); a pair is kept when it has more than ``min_matches`` matches (:222-223).

The reference runs N extractions and N(N-1)/2 single-pair matcher calls, moving every feature set to
the host and back.  Here the down-sampling, the extractions and all matches stay in HBM: the features
form one device table and the pairs go through ``LightGlueHIP.match_batch`` in batches (pair -> row
indirection); only the per-pair match counts come back.  With ``rank`` / ``world`` the pairs are sharded
like ``pipeline.PairMatchingPipeline`` does and the (disjoint) per-rank counts are summed with one all-reduce.

``do_geometric_verification`` (cv2 RANSAC on the low-res matches, :206-220) is not rebuilt.
"""
from __future__ import annotations

import ctypes
from itertools import combinations
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi
from .lightglue_hip import LightGlueHIP
from .superpoint_hip import SuperPointHIP

# pairs_generator.py:103-126
LOWRES_SP_CONF = {"nms_radius": 3, "max_keypoints": 2048, "keypoint_threshold": 0.0005, "remove_borders": 4, "fix_sampling": True}
LOWRES_LG_CONF = {"n_layers": 7, "depth_confidence": 0.9, "width_confidence": 0.95, "filter_threshold": 0.3}


def pairs_from_sequential(img_list: Sequence, overlap: int) -> List[tuple]:
    pairs = []
    for i in range(len(img_list)):
        for k in range(overlap):
            j = i + k + 1
            if j >= len(img_list):
                break
            pairs.append((img_list[i], img_list[j]))
    return pairs


def pairs_from_bruteforce(img_list: Sequence) -> List[tuple]:
    return list(combinations(img_list, 2))


def pairs_from_retrieval(query_names: Sequence[str], db_names: Sequence[str], query_desc, db_desc, num_matched: int,
                         min_score: Optional[float] = 0.0, device="cuda", lib=None) -> List[tuple]:
    """thirdparty/hloc/pairs_from_retrieval.py:49-70,108-112 on the device: global descriptors (N, D) -> similarity GEMM
    -> self / low-score masking -> top-``num_matched`` per query; returns (query, db) name pairs in the reference's order
    (query by query, best first).  Only the (nq, k) index table leaves the device."""
    lib = lib if lib is not None else capi.load()
    dev = torch.device(device)
    # device tensors (RetrievalPairSelector's descriptor table) are taken as they lie; anything else goes through numpy as before
    as_f32 = lambda x: x.to(torch.float32) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=torch.float32)  # noqa: E731
    q, d = as_f32(query_desc), as_f32(db_desc)
    nq, nd, D = q.shape[0], d.shape[0], q.shape[1]
    if nq == 0 or nd == 0:
        return []
    pad = (-D) % 32
    if pad:
        q, d = torch.nn.functional.pad(q, (0, pad)), torch.nn.functional.pad(d, (0, pad))
    k = min(int(num_matched), nd)   # torch.topk raises for k > nd; hloc callers keep num_matched <= number of images
    q, d = q.contiguous().to(dev), d.contiguous().to(dev)
    invalid = torch.from_numpy(np.array(query_names)[:, None] == np.array(db_names)[None]).to(torch.uint8).contiguous().to(dev)
    sim = torch.empty(nq, nd, dtype=torch.float32, device=dev)
    idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
    val = torch.empty(nq, k, dtype=torch.float32, device=dev)
    stream = capi.stream_ptr(dev)
    with capi.device_ctx(dev):   # launch on dev, not on the current device
        capi.check(lib, lib.dim_op_retrieval_topk(capi.ptr(q), nq, capi.ptr(d), nd, D + pad, capi.ptr(invalid), k,
                                                  ctypes.c_float(0.0 if min_score is None else float(min_score)), int(min_score is not None),
                                                  capi.ptr(sim), capi.ptr(idx), capi.ptr(val), stream))
    idx = idx.cpu().numpy()
    return [(query_names[i], db_names[j]) for i in range(nq) for j in idx[i] if j >= 0]


class LowresPairSelector:
    """``pairs_from_lowres`` with resident networks.  ``images``: grey float32 arrays (0..255) in list order."""

    def __init__(self, sp_state_dict, lg_state_dict, resize_max: int = 1000, min_matches: int = 20, pair_batch: int = 8,
                 device="cuda", lib=None, rank: int = 0, world: int = 1):
        self.resize_max, self.min_matches, self.pair_batch = int(resize_max), int(min_matches), int(pair_batch)
        self.device = torch.device(device)
        self.lib = lib if lib is not None else capi.load()
        self.rank, self.world = rank, world
        self._sp_sd, self._lg_sd = sp_state_dict, lg_state_dict
        self._sp: Optional[SuperPointHIP] = None
        self._sp_hw = (0, 0)
        self._lg: Optional[LightGlueHIP] = None

    def _stream(self):
        return capi.stream_ptr(self.device)

    def downsample(self, image: np.ndarray) -> torch.Tensor:
        """pairs_generator.py:141-146: size (w, h), scale = resize_max / max, rounded size, INTER_AREA, /255."""
        H, W = image.shape[:2]
        scale = self.resize_max / max(W, H)
        w, h = int(round(W * scale)), int(round(H * scale))
        src = torch.as_tensor(np.ascontiguousarray(image, dtype=np.float32)).to(self.device)
        dst = torch.empty(h, w, dtype=torch.float32, device=self.device)
        capi.check(self.lib, self.lib.dim_op_resize_area_f32(capi.ptr(src), H, W, capi.ptr(dst), h, w, 1, self._stream()))
        return dst

    def extract(self, images: Sequence[np.ndarray]):
        """Feature table of the down-sampled images: kpts [n, cap, 2], desc [n, cap, 256], n_kpts [n], size [n, 2]."""
        cap = 2048
        n = len(images)
        kt = torch.zeros(n, cap, 2, dtype=torch.float32, device=self.device)
        dt = torch.zeros(n, cap, 256, dtype=torch.float32, device=self.device)
        nt = torch.zeros(n, dtype=torch.int32, device=self.device)
        st = torch.ones(n, 2, dtype=torch.float32, device=self.device)
        for i, im in enumerate(images):
            small = self.downsample(im)
            h, w = small.shape
            if self._sp is None or h > self._sp_hw[0] or w > self._sp_hw[1]:
                self._sp_hw = (max(h, self._sp_hw[0], self.resize_max), max(w, self._sp_hw[1], self.resize_max))
                self._sp = SuperPointHIP(self._sp_sd, LOWRES_SP_CONF, max_batch=1, max_hw=self._sp_hw, capacity=cap,
                                         device=self.device, lib=self.lib)
            kp, _, de, nk = self._sp.extract_batch_guarded(small[None].contiguous())
            kt[i], dt[i], nt[i] = kp[0], de[0], nk[0]
            k = kp[0, : int(nk[0].item())]
            if k.numel():  # no image_size in the reference's call: LightGlue uses the keypoint extent (LGN:26-27)
                st[i] = 1 + k.max(0).values - k.min(0).values
        return kt, dt, nt, st

    def match_counts(self, table, pairs: Sequence[Tuple[int, int]]) -> np.ndarray:
        """len(matches) of every (i, j) in ``pairs`` (this rank's shard when world > 1, then all-gathered)."""
        kt, dt, nt, st = table
        if self._lg is None:
            self._lg = LightGlueHIP(self._lg_sd, LOWRES_LG_CONF, max_pairs=self.pair_batch, max_kpts=kt.shape[1], device=self.device, lib=self.lib)
        P = len(pairs)
        mine = list(range(self.rank, P, self.world))
        counts = torch.zeros(P, dtype=torch.int32, device=self.device)

        def run():  # all chunks are enqueued back to back; the fp16x3 range guard is read once for the whole shard
            out = None
            for s in range(0, len(mine), self.pair_batch):
                chunk = mine[s:s + self.pair_batch]
                pidx = torch.tensor([pairs[c] for c in chunk], dtype=torch.int32, device=self.device).contiguous()
                out = self._lg.match_batch(kt, dt, nt, st, pair_idx=pidx, n_pairs=len(chunk), out=out)  # the first chunk is the largest
                counts[torch.tensor(chunk, device=self.device)] = out["n_matches"][: len(chunk)]

        self._lg.guarded(run, "matching_lowres")
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(counts, op=dist.ReduceOp.SUM)  # shards are disjoint: the sum is the gather
        return counts.cpu().numpy()

    def select(self, names: Sequence, images: Sequence[np.ndarray]) -> List[tuple]:
        """pairs_from_lowres: the brute-force pairs (combinations order) with more than min_matches matches."""
        idx_pairs = list(combinations(range(len(names)), 2))
        if not idx_pairs:
            return []
        counts = self.match_counts(self.extract(images), idx_pairs)
        return [(names[i], names[j]) for (i, j), c in zip(idx_pairs, counts) if c > self.min_matches]


class RetrievalPairSelector:
    """The ``retrieval`` strategy (pairs_generator.py:327-339 -> image_retrieval.py) with a resident NetVLAD: hloc's
    ``extract_features.confs["netvlad"]`` preprocessing (RGB, ``resize_max`` 1024 with cv2 INTER_AREA, size rule ``int(round(x * scale))``,
    thirdparty/hloc/extract_features.py:200-205; /255), the global descriptors (netvlad_hip.NetVLADHIP), hloc's ``pairs_from_retrieval`` on the
    descriptor table as it lies in HBM, and image_retrieval.py:28-44's removal of duplicates.  ``images``: RGB float32 / uint8 arrays (0..255) in
    list order.  Same-sized images go through the network in batches of up to ``max_batch``; only the (n, num_matched) index table leaves the
    device."""

    def __init__(self, netvlad_state, resize_max: int = 1024, max_batch: int = 8, conf: Optional[dict] = None, device="cuda", lib=None):
        self.resize_max, self.max_batch = int(resize_max), int(max_batch)
        self.device = torch.device(device)
        self.lib = lib if lib is not None else capi.load()
        self._state, self._conf = netvlad_state, dict(conf or {})
        self._net = None
        self._net_hw = (0, 0)

    def _stream(self):
        return capi.stream_ptr(self.device)

    def _size(self, image: np.ndarray):
        """(h, w) the network sees: thirdparty/hloc/extract_features.py:200-205."""
        H, W = image.shape[:2]
        if max(H, W) <= self.resize_max:
            return H, W
        scale = self.resize_max / max(W, H)
        return int(round(H * scale)), int(round(W * scale))

    def preprocess(self, image: np.ndarray, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[H,W,3] 0..255 -> [h,w,3] in 0..1 on the device (into ``out`` when given); down-sampled with the area kernel when max(size) > resize_max.
        A non-finite pixel raises ValueError here, on the host: the network's clamp would read a NaN as 0 (include/dim_hip.h)."""
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError(f"RetrievalPairSelector: image of shape {tuple(image.shape)}, (H, W, 3) expected")
        host = np.ascontiguousarray(image, dtype=np.float32)
        if not np.isfinite(host).all():
            raise ValueError("RetrievalPairSelector: image holds a non-finite value")
        H, W = image.shape[:2]
        h, w = self._size(image)
        src = torch.as_tensor(host).to(self.device)
        if out is None:
            out = torch.empty(h, w, 3, dtype=torch.float32, device=self.device)
        if (h, w) == (H, W):
            torch.div(src, 255.0, out=out)
            return out
        planes = src.permute(2, 0, 1).contiguous()   # the area kernel takes single-channel planes
        dst = torch.empty(3, h, w, dtype=torch.float32, device=self.device)
        with capi.device_ctx(self.device):
            for c in range(3):
                capi.check(self.lib, self.lib.dim_op_resize_area_f32(capi.ptr(planes[c]), H, W, capi.ptr(dst[c]), h, w, 1, self._stream()))
        out.copy_(dst.permute(1, 2, 0))
        return out

    def describe(self, images: Sequence[np.ndarray]) -> torch.Tensor:
        """Descriptor table [n, dim] on the device, rows in list order.  Images are uploaded and preprocessed one batch at a time into one staging
        buffer per size, so the device holds a batch of images, not the list."""
        from .netvlad_hip import NetVLADHIP

        sizes = [self._size(im) for im in images]
        mh, mw = max(s[0] for s in sizes), max(s[1] for s in sizes)
        if self._net is None or mh > self._net_hw[0] or mw > self._net_hw[1]:
            self._net_hw = (max(mh, self._net_hw[0]), max(mw, self._net_hw[1]))
            self._net = NetVLADHIP(self._state, self._conf, max_batch=self.max_batch, max_hw=self._net_hw, device=self.device, lib=self.lib)
        by_size = {}
        for i, s in enumerate(sizes):
            by_size.setdefault(s, []).append(i)
        order = [i for idx in by_size.values() for i in idx]   # processing order: size by size; descriptors land in consecutive rows of `work`
        work = torch.empty(len(images), self._net.dim, dtype=torch.float32, device=self.device)

        def run():   # every batch is enqueued back to back; the fp16x3 range guard is read once for the whole list
            row = 0
            for (h, w), idx in by_size.items():
                stage = torch.empty(min(self.max_batch, len(idx)), h, w, 3, dtype=torch.float32, device=self.device)
                for s0 in range(0, len(idx), self.max_batch):
                    chunk = idx[s0:s0 + self.max_batch]
                    for j, i in enumerate(chunk):
                        self.preprocess(images[i], out=stage[j])
                    self._net.extract_batch(stage[:len(chunk)], out=work[row:row + len(chunk)])
                    row += len(chunk)

        self._net.guarded(run, "retrieval")
        if order == list(range(len(images))):
            return work
        inverse = torch.empty(len(order), dtype=torch.long)
        inverse[torch.tensor(order)] = torch.arange(len(order))
        return work[inverse.to(self.device)]

    def select(self, names: Sequence, images: Sequence[np.ndarray], num_matched: int = 10, min_score: Optional[float] = 0.0) -> List[tuple]:
        """(name, name) pairs: every image's ``num_matched`` most similar others, best first, query by query, similarities below ``min_score`` never
        (0, as pairs_from_retrieval.main hands it to pairs_from_score_matrix, thirdparty/hloc/pairs_from_retrieval.py:112: an image may get fewer
        pairs, or none); a pair that has already come out in either order is dropped (image_retrieval.py:34-42)."""
        if len(names) < 2:
            return []
        names = list(names)
        table = self.describe(images)
        pairs = pairs_from_retrieval(names, names, table, table, num_matched, min_score=min_score, device=self.device, lib=self.lib)
        seen, out = set(), []
        for a, b in pairs:
            key = tuple(sorted((a, b)))
            if key not in seen:
                seen.add(key)
                out.append((a, b))
        return out
