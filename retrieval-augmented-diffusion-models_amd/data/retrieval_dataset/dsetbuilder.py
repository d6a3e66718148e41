"""Native counterpart of the sampling-path methods of rdm/data/retrieval_dataset/dsetbuilder.py::DatasetBuilder:
load_embeddings / load_single_file / load_multi_files (:181-236), train_searcher (:534-619), search_k_nearest
(:478-518), embed (:461-473), and the `.searcher.search_batched / .search` surface of the ScaNN object
(:490, rdm/data/base.py:81); plus the database-construction side: build_data_pool (:317-437),
save_datapool (:238-259), reset_data_pool (:261-262) with the CLIP image tower running on the GPU.

The searcher is exact brute force on the GPU (the reference's ScaNN tree-AH is approximate): the
database is normalised and held in HBM as fp16 (dsetbuilder.py:574), a batch of queries streams it once.
numpy in / numpy out like the reference.
"""
import glob
import os
import time

import numpy as np
import torch

from ... import _lib


class HipSearcher(object):
    """Drop-in for the scann searcher object.  With `row0` / `group` the context holds only rows [row0, row0 + n_local) of the
    database (one shard per rank): every search runs on the local rows, the per-rank lists are merged in one exchange
    (parallel.merge_sharded_topk) and the answer -- global row ids -- is the same on every rank and the same as an unsharded search."""

    def __init__(self, ctx, dim, row0=0, group=None, sharded=False, n_local=None):
        self.ctx, self.dim, self.row0, self.group, self.sharded, self.n_local = ctx, dim, int(row0), group, bool(sharded), n_local

    def _search(self, q: torch.Tensor, k: int, allow=None, mask_of_query=None):
        """allow / mask_of_query: the row filter of Context.knn over THIS context's rows (sharded: every rank passes its local masks).  A
        query whose masks allow fewer than k rows over all shards gets (NO_ROW, -inf) in the places beyond them."""
        filt = {} if allow is None else {"allow": allow, "mask_of_query": mask_of_query}        # none given: today's call, unchanged
        if not self.sharded:
            return self.ctx.knn(q, k, **filt)
        from ... import parallel
        kl = min(k, self.n_local)
        idx, sc = self.ctx.knn(q, kl, f64=True, **filt)
        gid = idx.to(torch.int64) & 0xffffffff
        gid = torch.where(gid == _lib.NO_ROW, torch.full_like(gid, 2 ** 62), gid + self.row0)      # the library's "no row" is the merge's
        if kl < k:                                                  # a shard shorter than k: pad with "no row"
            pad = k - kl
            gid = torch.cat([gid, torch.full((gid.shape[0], pad), 2 ** 62, dtype=torch.int64, device=gid.device)], dim=1)
            sc = torch.cat([sc, torch.full((sc.shape[0], pad), float("-inf"), dtype=torch.float64, device=sc.device)], dim=1)
        gi, gs = parallel.merge_sharded_topk(gid, sc, k, self.group)
        gi = torch.where(gi >= 2 ** 62, torch.full_like(gi, _lib.NO_ROW), gi)
        return gi.to(torch.int32), gs.to(torch.float32)             # uint32 bits, like the unsharded call

    def search_batched(self, queries, final_num_neighbors=None, allow=None, mask_of_query=None, **kw):
        q = torch.as_tensor(np.ascontiguousarray(queries, dtype=np.float32))
        idx, dist = self._search(q, int(final_num_neighbors), allow, mask_of_query)
        return idx.cpu().numpy().view(np.uint32), dist.cpu().numpy()

    def search_batched_device(self, queries: torch.Tensor, k: int, allow=None, mask_of_query=None):
        """Device-resident variant (no host round trip): -> (idx int32-bits-of-uint32 [B,k], score f32 [B,k])."""
        return self._search(queries, k, allow, mask_of_query)

    def search(self, query, final_num_neighbors=None, **kw):
        i, d = self.search_batched(np.asarray(query)[None], final_num_neighbors)
        return i[0], d[0]


class DatasetBuilder(object):
    def __init__(self, saved_embeddings=None, k=20, retriever=None, retriever_config=None, ctx=None, device=0,
                 data_pool=None, load_patch_dataset=False, batch_size=100, max_pool_size=None, **ignored):
        self.k = k
        self.out_dir = ignored.get('out_dir')
        self.max_pool_size = max_pool_size
        self.batch_size = batch_size
        self.saved_embeddings = saved_embeddings
        self.load_patch_dataset = load_patch_dataset
        self.visualize = False
        self.retriever = retriever
        self.searcher = None
        self._subsets = {}                                  # name -> {"rows": sorted global row indices, "mask": device mask or None}
        self._dev_index = device if isinstance(device, int) else (torch.device(device).index or 0)
        self._ctx = ctx if ctx is not None else (retriever.model.ctx if retriever is not None else None)
        self.data_pool = {'embedding': [], 'img_id': [], 'patch_coords': []}
        if data_pool is not None:
            self.data_pool = {k_: np.asarray(v) for k_, v in data_pool.items()}
        elif saved_embeddings is not None:
            self.load_embeddings(saved_embeddings)

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.Context(self._dev_index)       # lazily: loading the npz shards needs no GPU
        return self._ctx

    # ---- dsetbuilder.py:181-236
    def load_single_file(self, saved_embeddings):
        compressed = np.load(saved_embeddings)
        self.data_pool = {key: compressed[key] for key in compressed.files}
        print('Finished loading of retrieval database of length', self.data_pool['embedding'].shape[0])

    def load_multi_files(self, data_archive):
        out = {key: [] for key in self.data_pool}
        for d in data_archive:
            for key in d.files:
                if key in out:
                    out[key].append(d[key])
        return out

    def load_embeddings(self, saved_embeddings):
        if os.path.isfile(saved_embeddings):
            return self.load_single_file(saved_embeddings)
        # the reference globs in filesystem order (dsetbuilder.py:222); here: deterministic, by the part index of
        # '<rows>x512-part_<i>.npz' (dsetbuilder.py:240-254) when present, else by name
        import re
        def part_key(f):
            m = re.search(r'part_(\d+)', os.path.basename(f))
            return (0, int(m.group(1)), f) if m else (1, 0, f)
        files = sorted(glob.glob(os.path.join(saved_embeddings, '*.npz')), key=part_key)
        assert len(files) > 0, f'No embedding shards (*.npz) under {saved_embeddings}'
        t0 = time.time()
        parts = self.load_multi_files([np.load(f) for f in files])
        self.data_pool = {key: np.concatenate(parts[key], axis=0) for key in parts if len(parts[key]) > 0}
        print(f'Finished loading of patch embeddings ({self.data_pool["embedding"].shape[0]} rows) in {time.time() - t0:.1f} s')

    # ---- dsetbuilder.py:534-619: "training" = upload + normalise on device
    def shard_rows(self, enabled=True, group=None):
        """[native] Hold only this rank's contiguous share of the database rows in HBM (for databases beyond one GPU's memory,
        SURVEY.md 8e); the host-side data_pool stays whole, like the reference's.  Takes effect at the next train_searcher()."""
        self._shard_rows, self._shard_group = bool(enabled), group
        self.searcher = None
        return self

    def train_searcher(self, k=None, metric=None, **ignored):
        emb = self.data_pool['embedding']
        row0, sharded, group = 0, bool(getattr(self, "_shard_rows", False)), getattr(self, "_shard_group", None)
        if sharded:
            from ... import parallel
            world, rank = parallel.world_rank(group)
            row0, row1 = parallel.shard_range(len(emb), world, rank)
            emb = emb[row0:row1]
        emb = np.ascontiguousarray(emb)
        if emb.dtype not in (np.float16, np.float32):
            emb = emb.astype(np.float32)
        self.ctx.db_load(emb)
        self.searcher = HipSearcher(self.ctx, emb.shape[1], row0=row0, group=group, sharded=sharded, n_local=emb.shape[0])
        for s in self._subsets.values():                    # the masks belong to the database just loaded (and to this rank's rows)
            s["mask"] = self._build_mask(s["rows"])
        return self.searcher

    # ---- [native] filtered retrieval: named row subsets of the resident database (a class, a style, a held-out split, a deny list)
    def _build_mask(self, rows):
        local = _lib.shard_row_mask(rows, self.searcher.row0, self.searcher.n_local) if self.searcher.sharded else rows
        return self.ctx.row_mask(local)

    def define_subset(self, name, rows_or_bool):
        """Name a subset of the database rows: an index array (duplicates allowed) or a boolean array over all rows.  The mask is built
        once and kept on the device (per shard when the rows are sharded) and rebuilt at train_searcher(); search_k_nearest(subset=name)
        and the models' db_subset= then search those rows only."""
        n = len(self.data_pool['embedding'])
        r = np.asarray(rows_or_bool.cpu().numpy() if isinstance(rows_or_bool, torch.Tensor) else rows_or_bool)
        if r.dtype == np.bool_:
            if r.shape != (n,):
                raise ValueError(f"define_subset({name!r}): a boolean subset must have one entry per database row ({n}), got {r.shape}")
            r = np.flatnonzero(r)
        if r.ndim != 1 or (r.size and not np.issubdtype(r.dtype, np.integer)):
            raise ValueError(f"define_subset({name!r}): row indices must be a 1-d integer array, got {r.dtype} {r.shape}")
        r = np.unique(r.astype(np.int64))
        if r.size and (r[0] < 0 or r[-1] >= n):
            raise ValueError(f"define_subset({name!r}): row indices must lie in [0, {n})")
        self._subsets[name] = {"rows": r, "mask": self._build_mask(r) if self.searcher is not None else None}
        return self

    def subsets(self):
        """-> {name: number of rows} of the defined subsets."""
        return {name: int(len(s["rows"])) for name, s in self._subsets.items()}

    def _subset_filter(self, subset, b):
        """subset: a name, or a list of b names / None (None: the whole database for that query) -> (allow, mask_of_query, names)."""
        names = [subset] * b if subset is None or isinstance(subset, str) else list(subset)
        if len(names) != b:
            raise ValueError(f"subset: one name per query ({b}), got {len(names)}")
        distinct = []
        for nm in names:
            if nm is not None and nm not in self._subsets:
                raise KeyError(f"subset {nm!r} is not defined (define_subset); defined: {sorted(self._subsets)}")
            if nm not in distinct:
                distinct.append(nm)
        words = _lib.knn_mask_words(self.ctx.db_size())
        masks = [torch.full((words,), -1, dtype=torch.int64, device=self.ctx.device) if nm is None else self._subsets[nm]["mask"] for nm in distinct]
        ids = np.array([distinct.index(nm) for nm in names], dtype=np.int32)
        return torch.stack(masks), ids, names

    def search_subset(self, query_embeddings, k, subset=None, short_ok=False):
        """searcher.search_batched over the rows of `subset` (_subset_filter) -> (nns uint32 [b,k], distances); a ValueError where a
        subset holds fewer than k rows -- before anything indexes the data pool with the "no row" id.
        short_ok [native]: a subset of 1 .. k - 1 rows does not raise; its queries come back with their rows followed by _lib.NO_ROW
        places (real_neighbours() counts and fills them), for a caller that masks the missing neighbours (the UNet's neighbour bias).  A
        subset without any row still raises."""
        if subset is None:
            return self.searcher.search_batched(query_embeddings, final_num_neighbors=k)
        allow, ids, names = self._subset_filter(subset, len(query_embeddings))
        nns, distances = self.searcher.search_batched(query_embeddings, final_num_neighbors=k, allow=allow, mask_of_query=ids)
        real = (np.asarray(nns) != _lib.NO_ROW).sum(axis=1)
        short = np.flatnonzero(real < (1 if short_ok else k))
        if short.size:
            nm = names[int(short[0])]
            raise ValueError(f"subset {nm!r} allows {len(self._subsets[nm]['rows'])} rows, fewer than k = {k} neighbours (query {int(short[0])})"
                             if not short_ok else f"subset {nm!r} allows no row at all (query {int(short[0])}): nothing to attend")
        return nns, distances

    @staticmethod
    def real_neighbours(nns):
        """[native] A search result with _lib.NO_ROW places (search_subset(short_ok=True)) -> (counts [b] of real neighbours, which
        lead each row; the index array with row 0 in the NO_ROW places, safe to index the data pool with; the boolean [b, k] of the
        real places)."""
        nns = np.asarray(nns)
        real = nns != _lib.NO_ROW
        return real.sum(axis=1).astype(np.int64), np.where(real, nns, 0), real

    # ---- dsetbuilder.py:461-473
    @torch.no_grad()
    def embed(self, batch, is_caption=False):
        if is_caption:
            from ...modules.custom_clip.tokenizer import tokenize
            tokens = torch.from_numpy(tokenize(list(batch), self.retriever.model.cfg.context_length))
            out = self.retriever.model.encode_text(tokens)
            bs = len(batch)
        else:
            batch = torch.as_tensor(batch)
            if batch.ndim == 4 and batch.shape[-1] in (1, 3):
                batch = batch.permute(0, 3, 1, 2)                    # b h w c -> b c h w (dsetbuilder.py:465)
            out = self.retriever(batch)
            bs = batch.shape[0]
        return out.cpu().numpy().reshape(bs, -1)

    # ---- dsetbuilder.py:261-262
    def reset_data_pool(self):
        self.data_pool = {key: [] for key in self.data_pool}

    # ---- dsetbuilder.py:238-259: '<rows>x<dim>[-<postfix>].npz', compressed, keys embedding / img_id / patch_coords (/ class_id)
    def save_datapool(self, postfix=None, out_dir=None):
        out_dir = out_dir or self.out_dir
        assert out_dir is not None, 'save_datapool needs an output directory (the reference hard-codes its NFS path)'
        pool = {key: np.concatenate([np.asarray(v) for v in self.data_pool[key]]) for key in self.data_pool if len(self.data_pool[key]) > 0}
        identifier = 'x'.join(str(s_) for s_ in pool['embedding'].shape)
        if postfix:
            identifier = identifier + '-' + postfix
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, identifier + '.npz')
        np.savez_compressed(path, **pool)
        self.saved_embeddings = out_dir
        return path

    # ---- dsetbuilder.py:317-437.  `loader` yields the reference's collated batches: {'patch': [b,(n,)h,w,c] in [-1,1],
    # 'img_id': [b(,n)], 'patch_coords': [b(,n),4]} (+ optional 'class_id'); the patches are embedded by the retriever
    # (CLIP image tower on the GPU incl. the bicubic 224x224 preprocessing, retrievers.py:83-95) and written in shards of
    # `chunk_size` rows named 'part_<i>' exactly like the shipped databases (scripts/download_databases.sh:6-15).
    def build_data_pool(self, loader, max_pool_size=None, chunk_size=None, save_embeddings=True, out_dir=None):
        self.out_dir = out_dir or self.out_dir
        max_pool_size = max_pool_size if max_pool_size is not None else (self.max_pool_size or float('inf'))
        self.data_pool = {'embedding': [], 'img_id': [], 'patch_coords': []}
        n_examples, part, files, kept = 0, 1, [], {'embedding': [], 'img_id': [], 'patch_coords': []}

        def flush():
            nonlocal part
            if len(self.data_pool['embedding']) == 0:
                return
            if save_embeddings:
                files.append(self.save_datapool(postfix=f'part_{part}' if chunk_size is not None else None))
            for key in self.data_pool:
                kept.setdefault(key, []).extend(self.data_pool[key])
            self.reset_data_pool()
            part += 1

        for batch in loader:
            if 'patch' not in batch:
                break
            patches = torch.as_tensor(batch['patch'])
            if patches.ndim == 5:                                     # b n h w c -> (b n) h w c (dsetbuilder.py:463-464)
                patches = patches.reshape((-1,) + tuple(patches.shape[2:]))
            emb = self.embed(patches)
            self.data_pool['embedding'].append(emb)
            self.data_pool['img_id'].append(np.asarray(batch['img_id']).reshape(emb.shape[0]))
            self.data_pool['patch_coords'].append(np.asarray(batch['patch_coords']).reshape(emb.shape[0], -1))
            if 'class_id' in batch:
                self.data_pool.setdefault('class_id', []).append(np.asarray(batch['class_id']).reshape(emb.shape[0]))
            n_examples += emb.shape[0]
            if chunk_size is not None and n_examples / chunk_size >= part:
                flush()
            if n_examples >= max_pool_size:
                break
        flush()
        self.data_pool = {key: np.concatenate([np.asarray(v) for v in kept[key]]) for key in kept if len(kept[key]) > 0}
        print(f'Finish extraction of {n_examples} feature embeddings')
        return files

    # ---- dsetbuilder.py:478-518
    def search_k_nearest(self, queries, k=None, is_caption=False, visualize=None, query_embedded=False, subset=None, short_ok=False):
        """subset [native]: a name given to define_subset, or a list of one name (or None = the whole database) per query: the exact
        k nearest among that subset's rows.  A subset of fewer than k rows is a ValueError -- unless short_ok [native]: then the
        missing places hold zero embeddings (img_ids / patch_coords: row 0's, meaningless there; nns keeps _lib.NO_ROW) and
        out['counts'] holds the number of real neighbours per query (k for everyone without a short subset)."""
        assert self.searcher is not None, 'Cannot search with uninitialized searcher'
        if k is None:
            k = self.k
        if not query_embedded:
            query_embeddings_ = self.embed(queries, is_caption=is_caption)
        else:
            query_embeddings_ = queries.cpu().numpy() if isinstance(queries, torch.Tensor) else np.asarray(queries)
        start = time.time()
        nns, distances = self.search_subset(query_embeddings_, k, subset, short_ok=short_ok)       # normalises on device (:487)
        end = time.time()
        counts, rows, real = self.real_neighbours(nns)
        emb = self.data_pool['embedding'][rows]
        if not real.all():
            emb = np.where(real[..., None], emb, np.zeros((), dtype=emb.dtype))
        out = {'embeddings': emb,
               'img_ids': self.data_pool['img_id'][rows] if len(self.data_pool.get('img_id', [])) else None,
               'patch_coords': self.data_pool['patch_coords'][rows] if len(self.data_pool.get('patch_coords', [])) else None,
               'queries': queries, 'exec_time': end - start, 'nns': nns, 'distances': distances,
               'q_embeddings': query_embeddings_}
        if short_ok:
            out['counts'] = counts
        if visualize if visualize is not None else self.visualize:
            raise NotImplementedError("nn_patches visualisation needs the raw OpenImages JPEGs (out of scope, SURVEY.md §2 #8)")
        return out
