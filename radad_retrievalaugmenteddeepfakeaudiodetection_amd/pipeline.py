"""Hot-path shell: the two pipeline methods whose loops this build collapses, with the reference's signatures
(pipeline.py:392-414 process_audio_batch, :449-532 retrieve_similar_vectors).  Training, metrics, plots, wandb
and the CLI stay in the reference; this class only wires segment -> embed -> retrieve.
"""
import os
from typing import List, Optional, Sequence

import numpy as np

from .feature_extractor import build_feature_extractor
from .pooling import TemporalPyramidPooling
from .segmenter import AudioSegmenter
from .vector_database import VectorDatabase


class HotPathPipeline:
    """The slice of DeepfakeDetectionPipeline.__init__ (pipeline.py:70-93) the hot path needs."""

    def __init__(self, config, feature_extractor=None):
        import torch
        self.config = config
        self.device = torch.device(config.device)
        self.audio_segmenter = AudioSegmenter(config)                                   # pipeline.py:78
        self.feature_extractor = feature_extractor or build_feature_extractor(config)   # pipeline.py:81
        config.feature_dim = self.feature_extractor.feature_dim                         # pipeline.py:85
        self.tpp = TemporalPyramidPooling(config)                                       # pipeline.py:89
        self.vector_db = VectorDatabase(config)                                         # pipeline.py:90
        self.training_file_ids = set()

    # ---- segment + embed --------------------------------------------------------------------------------
    def embed_waves(self, wave, clip_offsets: Sequence[int]):
        """Device-resident form: `wave` holds the clips back to back on the GPU -> [B, D]."""
        fe = self.feature_extractor
        if hasattr(fe, "embed_clips"):
            return fe.embed_clips(wave, clip_offsets)           # one fused pass (csrc/embed.hip)
        # protocol-only extractor: the reference's composition, stage by stage (pipeline.py:402-414)
        import torch
        host = wave.detach().cpu().numpy()
        pooled = []
        for b in range(len(clip_offsets) - 1):
            segs = self.audio_segmenter.segment_audio(host[clip_offsets[b]:clip_offsets[b + 1]])
            feats = [t.to(self.device) for t in fe.extract_features(segs)]
            pooled.append(torch.mean(self.tpp.pool_features_batch(feats), dim=0))
        return torch.stack(pooled)

    def process_audio_batch(self, audio_paths: List[str], audio_dataset) -> "torch.Tensor":
        """pipeline.py:392-414.  `audio_dataset` only needs `.load_audio(path) -> 1-D float array`."""
        import torch
        waves = []
        for path in audio_paths:
            wav = audio_dataset.load_audio(path)
            if wav is None:
                raise RuntimeError(f"Failed to load '{path}'")       # pipeline.py:398-399
            wav = np.asarray(wav, np.float32)
            if wav.ndim > 1:
                raise ValueError("Expected 1D audio array")          # segmenter.py:18-19
            waves.append(wav)
        offs = np.zeros(len(waves) + 1, np.int64)
        np.cumsum([len(w) for w in waves], out=offs[1:])
        flat = torch.from_numpy(np.concatenate(waves) if waves else np.zeros(0, np.float32)).to(self.device)
        return self.embed_waves(flat, offs)                          # [batch, tpp_output_dim]

    # ---- build the store ------------------------------------------------------------------------------------
    def build_vector_database(self, batches, audio_dataset, save: bool = True):
        """pipeline.py:416-447 without the host round trip: every batch is embedded on the GPU and appended to the
        HBM-resident store as a device tensor (the reference does .cpu().numpy() -> np.vstack -> index.add).
        `batches` yields dicts like the reference's DataLoader does: {'path': [...], 'label': [...], 'metadata': ...}."""
        self.training_file_ids.clear()
        n = 0
        for batch in batches:
            paths = list(batch["path"])
            vecs = self.process_audio_batch(paths, audio_dataset)            # [b, D] on the device
            labels = [int(l) if not hasattr(l, "item") else int(l.item()) for l in batch["label"]]
            speakers = self._extract_batch_speakers(batch.get("metadata"), len(paths))
            self.training_file_ids.update(os.path.basename(p) for p in paths)     # pipeline.py:437-438
            self.vector_db.add_vectors(vecs, paths, labels, {"speaker_id": speakers})
            n += len(paths)
        if save:
            self.vector_db.save()                                             # pipeline.py:446
        return n

    def remove_files(self, paths) -> int:
        """Act on an audit (near_duplicates, validate_no_leakage): take every stored row of these files out of the store, in place
        (VectorDatabase.remove_files: matched by basename), and their basenames out of training_file_ids.  -> rows removed."""
        removed = self.vector_db.remove_files(paths)                # (raises before anything changes on a store that cannot remove)
        self.training_file_ids.difference_update(os.path.basename(p) for p in ([paths] if isinstance(paths, str) else paths))
        return removed

    @staticmethod
    def _extract_batch_speakers(metas, batch_size):
        """the speaker_id column the reference keeps beside each vector (pipeline.py:433-443)"""
        if isinstance(metas, dict) and "speaker_id" in metas:
            sp = list(metas["speaker_id"])
            return (sp + ["unknown"] * batch_size)[:batch_size]
        if isinstance(metas, (list, tuple)) and len(metas) == batch_size:
            return [m.get("speaker_id", "unknown") if isinstance(m, dict) else "unknown" for m in metas]
        return ["unknown"] * batch_size

    # ---- audit by content ---------------------------------------------------------------------------------
    def near_duplicates(self, query_vectors, thresh: float, max_per_query: int = 128, query_paths: Optional[List[str]] = None,
                        exact_exclusion: bool = False, exclude: str = "file", query_speakers: Optional[List[str]] = None,
                        probed: bool = False, probed_exclusion: bool = False):
        """Per query the stored rows within `thresh` of it (VectorDatabase.range_search_batch: cosine / inner product > thresh, or
        squared L2 < thresh, exactly), as a list of (path, label, score), best first, at most max_per_query.  The content
        counterpart of validate_no_leakage (pipeline.py:1105-1110), which compares basenames and so passes a re-encoded or renamed
        copy of a training clip.  With `query_paths`, entries whose basename equals the query's own are dropped (the file itself),
        a copy under another name stays.
        That default filters AFTER the search: the query's own rows have taken slots of max_per_query by then, and nothing says how
        many other rows exist.  exact_exclusion=True runs the exclusion IN the search
        (VectorDatabase.range_search_excluding_per_query_batch) and returns (hits, counts): counts[j] is the exact number of admissible
        rows within the radius, and all max_per_query slots go to admissible rows.  exclude="file": query j excludes the rows whose
        basename is that of query_paths[j]; exclude="speaker": the rows whose stored speaker_id metadata equals query_speakers[j]
        (leave-one-speaker-out).
        probed=True (IVF stores; a ValueError on a flat one): the same lists from the rows of the probed lists
        (VectorDatabase.range_search_probed_batch, config.vector_db_nprobe; squared L2 < thresh) -- the audit on a store that is too
        large to scan whole.  Not offered with exact_exclusion (the flat store's call); its own switch is
        probed_exclusion=True (only with probed=True): the exclusion runs inside the IVF list scans
        (VectorDatabase.range_search_probed_excluding_per_query_batch) and the call returns (hits, counts) as exact_exclusion does --
        counts[j] the exact number of admissible rows of query j's probed lists within the radius, every slot an admissible row;
        exclude="file" and exclude="speaker" as above.  Without it the probed audit filters by basename after the search."""
        if exclude not in ("file", "speaker"):
            raise ValueError(f"exclude must be 'file' or 'speaker', got {exclude!r}")
        if probed and exact_exclusion:
            raise ValueError("near_duplicates: exact_exclusion is not offered with probed=True (an IVF range search takes no exclusion sets)")
        if probed_exclusion and not probed:
            raise ValueError("near_duplicates: probed_exclusion needs probed=True (a flat store has exact_exclusion)")
        if probed_exclusion:
            return self._near_duplicates_excluding(query_vectors, thresh, max_per_query, query_paths, exclude, query_speakers, probed=True)
        if exact_exclusion:
            return self._near_duplicates_excluding(query_vectors, thresh, max_per_query, query_paths, exclude, query_speakers)
        search = self.vector_db.range_search_probed_batch if probed else self.vector_db.range_search_batch
        lims, dist, idx = search(query_vectors, thresh, max_per_query=max_per_query)[:3]
        if hasattr(lims, "cpu"):
            lims, dist, idx = lims.cpu().numpy(), dist.cpu().numpy(), idx.cpu().numpy()
        base = self.vector_db.index.id_base if hasattr(self.vector_db.index, "id_base") else 0
        out = []
        for j in range(len(lims) - 1):
            own = os.path.basename(query_paths[j]) if query_paths is not None else None
            hits = []
            for d, i in zip(dist[lims[j]:lims[j + 1]], idx[lims[j]:lims[j + 1]]):
                path = self.vector_db.vector_paths[int(i) - base]
                if own is not None and os.path.basename(path) == own:
                    continue
                hits.append((path, self.vector_db.vector_labels[int(i) - base], float(d)))
            out.append(hits)
        return out

    @staticmethod
    def _speaker_tag(speaker) -> int:
        """stable 63-bit tag of a speaker id, as path_tag is of a basename"""
        import hashlib
        h = hashlib.blake2b(str(speaker).encode("utf-8", "surrogatepass"), digest_size=8).digest()
        return int.from_bytes(h, "little") & 0x7FFFFFFFFFFFFFFF

    def _near_duplicates_excluding(self, query_vectors, thresh, max_per_query, query_paths, exclude, query_speakers, probed=False):
        import torch
        from .vector_database import path_tag
        vdb = self.vector_db
        nq = 1 if getattr(query_vectors, "ndim", 2) == 1 else len(query_vectors)
        what = "probed_exclusion" if probed else "exact_exclusion"
        if exclude == "file":
            if query_paths is None:
                raise ValueError(f"{what} with exclude='file' needs query_paths")
            row_tags, q_tags = None, [path_tag(p) for p in query_paths]               # (the per-row basename tags the store keeps)
        else:
            if query_speakers is None:
                raise ValueError(f"{what} with exclude='speaker' needs query_speakers")
            stored = vdb.vector_metadata.get("speaker_id") if isinstance(vdb.vector_metadata, dict) else None
            if stored is None or len(stored) != len(vdb.vector_paths):
                raise ValueError("exclude='speaker' needs the speaker_id metadata of every stored row")
            cache = getattr(self, "_speaker_tags", None)
            if cache is None or cache.numel() != len(stored):
                cache = self._speaker_tags = torch.tensor([self._speaker_tag(s_) for s_ in stored], dtype=torch.int64,
                                                          device=torch.device("cuda", vdb.device_id))
            row_tags, q_tags = cache, [self._speaker_tag(s_) for s_ in query_speakers]
        if len(q_tags) != nq:
            raise ValueError(f"{nq} queries, {len(q_tags)} {'query_paths' if exclude == 'file' else 'query_speakers'}")
        search = vdb.range_search_probed_excluding_per_query_batch if probed else vdb.range_search_excluding_per_query_batch
        lims, dist, idx, counts = search(query_vectors, thresh, query_tags=q_tags, max_per_query=max_per_query, return_counts=True, row_tags=row_tags)
        if hasattr(lims, "cpu"):
            lims, dist, idx, counts = lims.cpu().numpy(), dist.cpu().numpy(), idx.cpu().numpy(), counts.cpu().numpy()
        base = vdb.index.id_base if hasattr(vdb.index, "id_base") else 0
        out = [[(vdb.vector_paths[int(i) - base], vdb.vector_labels[int(i) - base], float(d))
                for d, i in zip(dist[lims[j]:lims[j + 1]], idx[lims[j]:lims[j + 1]])] for j in range(len(lims) - 1)]
        return out, counts

    # ---- retrieve -----------------------------------------------------------------------------------------
    def retrieve_similar_vectors(self, query_vectors, query_paths: Optional[List[str]] = None, exclude_self: bool = True,
                                 return_info: bool = False, return_distances: bool = False):
        """pipeline.py:449-532 with the same four return arities.  Search, basename exclusion (:491-509, through
        per-row tags), compaction to K, label and neighbour-row gathers (:503) all stay on the device; nothing is
        copied to the host unless `return_info` asks for the path strings.  Unfilled search slots (id -1) are skipped
        instead of wrapping to vector_paths[-1] as the reference does (:495)."""
        import torch
        B = query_vectors.shape[0]
        K = int(self.config.top_k)
        D = self.tpp.get_output_dim()

        def pack(vec, lbl, paths, dist):
            if return_info and return_distances:
                return vec, lbl, paths, dist
            if return_info:
                return vec, lbl, paths
            if return_distances:
                return vec, lbl, dist
            return vec, lbl

        index = self.vector_db.index
        if index is None or getattr(index, "ntotal", 0) == 0:                   # pipeline.py:465-476
            return pack(torch.zeros(B, K, D, device=self.device), torch.zeros(B, K, device=self.device),
                        [[""] * K for _ in range(B)], torch.full((B, K), float("nan"), device=self.device))

        exclude_ids = set()
        if exclude_self and query_paths is not None:
            exclude_ids = {os.path.basename(p) for p in query_paths}            # pipeline.py:463
        k_search = K + (10 if exclude_self else 0)                              # pipeline.py:478
        q = query_vectors.detach().to(self.device, torch.float32)
        # config.exact_exclusion (opt-in, this build's): the K nearest rows that are NOT excluded, however many excluded rows sit in
        # front of them (VectorDatabase.search_excluding), instead of the reference's "search K + 10, drop, pad" below
        from .vector_database import HipFlatIndex, HipIVFFlatIndex, path_tag
        exact_excl = bool(getattr(self.config, "exact_exclusion", False)) and exclude_self
        # config.exclusion_scope "query" (opt-in): clip i excludes its OWN basename and nothing else (VectorDatabase.
        # search_excluding_per_query), so what a clip retrieves does not depend on its batch; "batch" is the reference's union (:463)
        scope = getattr(self.config, "exclusion_scope", "batch")
        if scope not in ("batch", "query"):
            raise ValueError(f"config.exclusion_scope must be 'batch' or 'query', got {scope!r}")
        per_query = scope == "query" and exclude_self
        # config.ivf_exact_exclusion (opt-in): the same for an IVF store, among the rows of the probed lists
        # (VectorDatabase.search_probed_excluding, with scope "query" search_probed_excluding_per_query); a flat store ignores it
        ivf_excl = bool(getattr(self.config, "ivf_exact_exclusion", False)) and exclude_self and isinstance(index, HipIVFFlatIndex)
        if exact_excl and not isinstance(index, HipFlatIndex):
            raise ValueError("config.exact_exclusion: exclusion-aware search is flat and single-handle only (vector_db_index_type 'L2' or 'IP'); "
                             "an IVF store takes config.ivf_exact_exclusion")
        if per_query and not exact_excl and not ivf_excl:
            raise ValueError("config.exclusion_scope 'query' needs config.exact_exclusion (flat stores) or config.ivf_exact_exclusion (IVF "
                             "stores): the over-fetch-and-drop path excludes the batch's union")
        # config.exclusion_in_scan (opt-in, with exact_exclusion, scope "batch", a flat store): the admission test inside the certified
        # tile scan (VectorDatabase.search_excluding_in_scan) -- for exclusion sets that cover most of the store (training_file_ids,
        # pipeline.py:500-502), where no over-fetch proves a query
        in_scan = bool(getattr(self.config, "exclusion_in_scan", False)) and exact_excl
        if in_scan and per_query:
            raise ValueError("config.exclusion_in_scan excludes one set for the batch (a bias is per row, not per (row, query)): "
                             "config.exclusion_scope 'query' takes search_excluding_per_query, without exclusion_in_scan")
        # config.exclusion_per_query_in_scan (opt-in, with exact_exclusion, scope "query", a flat store): the per-query search on the
        # certified tile scan (VectorDatabase.search_excluding_per_query_in_scan) -- for basenames carried by so many rows that no
        # k_fetch proves a query
        pq_in_scan = bool(getattr(self.config, "exclusion_per_query_in_scan", False))
        if pq_in_scan and exclude_self and not (exact_excl and per_query):
            raise ValueError("config.exclusion_per_query_in_scan needs config.exact_exclusion and config.exclusion_scope 'query' on a flat "
                             "store (one set for the batch inside the scan is config.exclusion_in_scan)")
        if per_query and query_paths is None:
            raise ValueError("config.exclusion_scope 'query' needs query_paths: a query excludes its own basename")
        if per_query and len(query_paths) != B:
            raise ValueError(f"config.exclusion_scope 'query' needs one path per query ({B}), got {len(query_paths)}")
        dists_t = idxs_t = None
        if not exact_excl and not ivf_excl:
            try:
                dists_t, idxs_t = self.vector_db.search_batch(q, k=k_search)
            except Exception:                                                   # pipeline.py:481-483: swallow, return padding
                dists_t = idxs_t = None

        # exclusion + compaction + gathers on the device (csrc/knn.hip k_filter_topk, k_gather_rows): basenames are
        # compared through their 63-bit tags, so the only per-row host work left is building the optional path lists
        excl = None
        if exclude_self:
            names = exclude_ids if query_paths is not None else getattr(self, "training_file_ids", set())
            if names:
                excl = torch.tensor(sorted({path_tag(n) for n in names}), dtype=torch.int64, device=self.device)
        if exact_excl or ivf_excl:
            own = None
            if per_query:
                own = torch.tensor([[path_tag(os.path.basename(p))] for p in query_paths], dtype=torch.int64, device=self.device)
            if ivf_excl:
                if per_query:
                    dist_t, chosen_t = self.vector_db.search_probed_excluding_per_query(q, K, own)
                else:
                    dist_t, chosen_t = self.vector_db.search_probed_excluding(q, K, excl)
            elif per_query and pq_in_scan:
                dist_t, chosen_t = self.vector_db.search_excluding_per_query_in_scan(q, K, own)
            elif per_query:
                k_fetch = getattr(self.config, "exclusion_k_fetch", K + 10)
                dist_t, chosen_t = self.vector_db.search_excluding_per_query(q, K, own, k_fetch=K + 10 if k_fetch is None else int(k_fetch))
            elif in_scan:
                dist_t, chosen_t = self.vector_db.search_excluding_in_scan(q, K, excl)
            else:
                k_fetch = getattr(self.config, "exclusion_k_fetch", K + 10)
                dist_t, chosen_t = self.vector_db.search_excluding(q, K, excl, k_fetch=K + 10 if k_fetch is None else int(k_fetch))
            if chosen_t.shape[1] < K:                                           # (a store of fewer than K rows: k was clamped to it)
                pad = K - chosen_t.shape[1]
                chosen_t = torch.cat([chosen_t, torch.full((B, pad), -1, dtype=torch.int64, device=self.device)], dim=1)
                dist_t = torch.cat([dist_t, torch.full((B, pad), float("nan"), device=self.device)], dim=1)
        else:
            if idxs_t is None:
                idxs_t = torch.zeros((B, 0), dtype=torch.int64, device=self.device)
                dists_t = torch.zeros((B, 0), dtype=torch.float32, device=self.device)
            dist_t, chosen_t = self.vector_db.filter_hits(dists_t, idxs_t, K, excl)
        valid = chosen_t >= 0
        rows_t = (chosen_t - index.id_base).clamp(min=0)
        lbl_t = torch.where(valid, self.vector_db.labels_device()[rows_t], torch.zeros((), device=self.device))   # 0.0 pad (:513)
        all_paths = None
        if return_info:
            paths_db = self.vector_db.vector_paths
            all_paths = [[paths_db[i - index.id_base] if i >= 0 else "" for i in row] for row in chosen_t.cpu().tolist()]
        vec_tensor = index.reconstruct_batch(chosen_t)                          # [B,K,D], zeros where id == -1 (pipeline.py:512)
        return pack(vec_tensor, lbl_t, all_paths, dist_t)

    # ---- the online path ------------------------------------------------------------------------------------
    def predict(self, audio_path: str, audio_dataset, radad_model, threshold: float = 0.5):
        """pipeline.py:1038-1103 for ONE clip: segment -> embed (:1047) -> retrieve with the clip's own basename excluded (:1049-1051)
        -> when that leaves nothing, retrieve again WITHOUT the exclusion (:1052-1055) -> RADADModel (:1076) -> sigmoid -> the
        reference's result dict (:1096-1103).  `audio_dataset` needs `.load_audio(path)` (the reference builds an AudioDataset
        around librosa, :1043); `radad_model` is this build's RADADModel (inference forward, csrc/proj.hip) or any module with the
        reference's forward(retrieved_vectors, tpp_vector).  Everything between the loaded samples and the logit stays on the GPU."""
        import logging
        import torch
        index = self.vector_db.index
        if index is None or getattr(index, "ntotal", 0) == 0:
            logging.warning("Vector DB is empty or not loaded. Retrieval will return zero neighbors.")      # :1039-1040
        radad_model.eval()                                                                                  # :1042
        with torch.no_grad():
            tpp_vec = self.process_audio_batch([audio_path], audio_dataset)                                 # [1, D]
            vecs, lbls, npaths = self.retrieve_similar_vectors(tpp_vec, query_paths=[audio_path], exclude_self=True, return_info=True)
            if torch.count_nonzero(vecs) == 0:                                                              # :1052
                vecs, lbls, npaths = self.retrieve_similar_vectors(tpp_vec, query_paths=[audio_path], exclude_self=False,
                                                                   return_info=True)
            if vecs.ndim == 2:                                                                              # :1057-1060
                vecs = vecs.unsqueeze(1)
            elif vecs.ndim == 1:
                vecs = vecs.unsqueeze(0).unsqueeze(1)
            logits = radad_model(vecs, tpp_vec)                                                             # :1076
            if logits.ndim == 1:
                logits = logits.unsqueeze(-1)
            flat = logits.detach().float().view(-1)
            prob = torch.sigmoid(flat).mean().item()                                                        # :1082
            pred = "spoof" if prob >= float(threshold) else "bona-fide"                                     # :1083
            logit = flat.mean().item()
            neigh_labels = [int(x) for x in lbls.squeeze(0).detach().cpu().tolist()] if isinstance(lbls, torch.Tensor) else \
                (list(lbls[0]) if isinstance(lbls, list) and len(lbls) else [])                             # :1087-1090
            neigh_paths = npaths[0] if isinstance(npaths, list) and len(npaths) else []
            retrieved = [{"file": os.path.basename(pth) if pth else "", "path": pth, "label": lab}
                         for lab, pth in zip(neigh_labels, neigh_paths)]
            return {"prediction": pred, "probability_spoof": float(prob), "logit": float(logit), "retrieved_labels": neigh_labels,
                    "retrieved_files": [r["file"] for r in retrieved], "retrieved": retrieved}
