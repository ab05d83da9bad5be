"""TGN orchestration over the HIP hot path (mirror of model/tgn_model.py:14-232).

``compute_temporal_embeddings`` / ``compute_edge_probabilities`` keep the
reference's signatures (numpy batches in, tensors out) and its exact ordering
of embedding, message store and memory update.  ``step_device`` is the same
eval-mode protocol with device-resident inputs and no host synchronisation:
it is what bench.py times.
"""
import collections
import ctypes as C
import logging

import numpy as np
import torch

from . import _capi
from ._capi import check, lib, ptr, stream_ptr
from .losses import _HipLinkBCE, link_bce_loss, listwise_loss
from .modules import Memory, MergeLayer, TimeEncode, _HipLinkScore, _HipRankScore, get_embedding_module, get_memory_updater


def link_score_plan(device_type, dtype, H, fused_scoring=True):
    """Which scorer a training step runs (pure host code, in the style of the library's embed_kernel_plan): "hip" --
    _HipLinkScore -- when ``fused_scoring`` is on, the embeddings are float32 on the GPU and the hidden width is one the
    kernels take (H % 4 == 0, 4 <= H <= 768: zt_affinity_train_workspace_bytes); else "torch", MergeLayer's composition."""
    if not fused_scoring or device_type != "cuda" or dtype != torch.float32:
        return "torch"
    return "hip" if (H % 4 == 0 and 4 <= H <= 768) else "torch"


def rank_score_plan(device_type, dtype, H, fused_scoring=True):
    """Which one-vs-many scorer a ranking training step runs (pure host code, as link_score_plan): "hip" -- _HipRankScore --
    when ``fused_scoring`` is on, the embeddings are float32 on the GPU and the hidden width is one zt_affinity_rank_train_*
    takes (H % 4 == 0, 4 <= H <= 4352: zt_affinity_rank's widths); else "torch", MergeLayer's composition."""
    if not fused_scoring or device_type != "cuda" or dtype != torch.float32:
        return "torch"
    return "hip" if (H % 4 == 0 and _capi.RANK_MIN_H <= H <= _capi.RANK_MAX_H) else "torch"


def absent_columns(absent, n_cols):
    """bool [Q, n_cols] of absent bits [Q, W] (include/zebra_amd.h, zt_affinity_topk_masked): True where bit c & 31 of word
    c >> 5 is set for column c"""
    col = torch.arange(n_cols, device=absent.device, dtype=torch.int64)
    words = absent.to(torch.int64).index_select(1, col >> 5)
    return ((words >> (col & 31).unsqueeze(0)) & 1) != 0


class TGN(torch.nn.Module):
    def __init__(self, neighbor_finder, node_features, edge_features, device, n_layers=2, n_heads=2, dropout=0.1,
                 use_memory=False, node_dimension=100, time_dimension=100, memory_dimension=100,
                 embedding_module_type="diffusion", message_function="identity", n_neighbors=None,
                 aggregator_type="last", memory_updater_type="gru", use_destination_embedding_in_message=False,
                 use_source_embedding_in_message=False, args=None):
        super().__init__()
        if message_function != "identity":
            raise ValueError("the reference only runs with the identity message function (tgn_model.py:64)")
        if use_destination_embedding_in_message or use_source_embedding_in_message:
            raise ValueError("embedding-in-message variants are not on the accelerated path")
        self.batch_counter = 0
        self.n_layers = n_layers
        self.neighbor_finder = neighbor_finder
        self.device = torch.device(device)
        self.logger = logging.getLogger(__name__)
        self.args = args
        self.test_mode = False

        if torch.is_tensor(edge_features):
            self.edge_raw_features = edge_features.to(self.device, torch.float32).contiguous()
        else:
            self.edge_raw_features = torch.from_numpy(np.asarray(edge_features).astype(np.float32)).to(self.device)
        self.n_edge_features = self.edge_raw_features.shape[1]
        self.n_nodes = args.n_nodes
        self.time_dimension = time_dimension
        self.memory_dimension = memory_dimension
        self.embedding_dimension = node_dimension
        self.n_node_features = self.embedding_dimension
        self.n_neighbors = n_neighbors
        self.embedding_module_type = embedding_module_type
        self.use_destination_embedding_in_message = use_destination_embedding_in_message
        self.use_source_embedding_in_message = use_source_embedding_in_message

        self.time_encoder = TimeEncode(dimension=self.time_dimension)
        self.use_memory = use_memory
        raw_message_dimension = 2 * self.memory_dimension + self.n_edge_features + self.time_dimension
        message_dimension = raw_message_dimension
        self.memory = Memory(n_nodes=self.n_nodes, memory_dimension=self.memory_dimension,
                             input_dimension=message_dimension, message_dimension=message_dimension,
                             device=self.device,
                             reference_compat_aliasing=getattr(args, "reference_compat_aliasing", False))
        self.memory_updater = get_memory_updater(module_type=memory_updater_type, message_dimension=message_dimension,
                                                 memory_dimension=self.memory_dimension, device=self.device)
        self.embedding_module = get_embedding_module(
            module_type=embedding_module_type, node_features=None, edge_features=self.edge_raw_features,
            memory=self.memory, neighbor_finder=self.neighbor_finder, time_encoder=self.time_encoder,
            n_layers=self.n_layers, n_node_features=self.n_node_features, n_edge_features=self.n_edge_features,
            n_time_features=self.time_dimension, embedding_dimension=self.embedding_dimension, device=self.device,
            n_heads=n_heads, dropout=dropout, use_memory=use_memory, n_neighbors=self.n_neighbors, args=args,
            num_nodes=self.n_nodes)
        hidden_dim = self.n_node_features * (len(args.alpha_list) + 1)
        self.affinity_score = MergeLayer(hidden_dim, hidden_dim, hidden_dim, 1)
        # training: the scorer's forward and backward on the HIP kernels (score_train); False: torch's MergeLayer under autograd
        self.fused_scoring = True
        # device scratch of the message-store kernel: last occurrence per node (all -1 between calls)
        self._scratch = torch.full((self.n_nodes,), -1, dtype=torch.int32, device=self.device)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.reset_timer()

    def reset_timer(self):
        self.t_get_message = self.t_store_message = self.t_clear_message = self.t_message = 0
        self.t_embedding = self.t_get_memory = self.t_update_memory = self.t_temporal = self.t_score = 0
        self.n_update_memory = 0
        self.embedding_module.t_tppr = 0

    # ------------------------------------------------------------------ device protocol
    def store_messages_device(self, src_d, dst_d, ts_d, eidx_d, pos_range=None):
        """get_raw_messages + store_raw_messages (tgn_model.py:204-226) on the device.
        ``pos_range`` = (lo, hi) restricts the work to winners at batch positions lo..hi-1.
        The touched nodes are exactly those whose flag is set afterwards; the GRU update
        finds them from the (duplicated) endpoint list, no compaction needed here."""
        B = src_d.numel()
        lo, hi = pos_range if pos_range is not None else (0, 2 * B)
        m = self.memory
        check(lib().zt_store_messages_range(ptr(m.memory), ptr(m.last_update), ptr(self.edge_raw_features),
                                      ptr(self.time_encoder.w.weight), C.c_int64(m.n_nodes),
                                      C.c_int64(self.edge_raw_features.shape[0]), C.c_int32(self.memory_dimension),
                                      C.c_int32(self.n_edge_features), C.c_int32(self.time_dimension), ptr(src_d),
                                      ptr(dst_d), ptr(ts_d), ptr(eidx_d), C.c_int64(B), C.c_int64(lo), C.c_int64(hi),
                                      ptr(m.messages),
                                      ptr(m.timestamps), ptr(m._flag_buf), ptr(self._scratch), None,
                                      None, ptr(self._status), stream_ptr()), "zt_store_messages")
        return B

    # ------------------------------------------------------------------ link scorer (tgn_model.py:185-188) on the device
    def _affinity_state(self, max_B, who="direct"):
        """(workspace, weights struct, weights_ready) of the HIP scorer for one CONSUMER -- "direct": score_device, which
        packs the weights in the call that finds them changed; "pipe": the native pipeline, which packs them in its next
        whole-batch step, on its own stream -- ; None when the hidden width has no kernel (zt_affinity_workspace_bytes: H % 4 == 0
        and 4 <= H <= 768, the training scorer's widths).  Each consumer has its own
        workspace (packed weights, partial scores, arrival counters) and its own packed-for key: the two pack at different
        times and run on different streams (round-4 advisor)."""
        a = self.affinity_score
        H = a.fc1.weight.shape[0]
        need = lib().zt_affinity_workspace_bytes(C.c_int64(max(1, max_B)), C.c_int32(H))
        if need < 0:
            return None
        allst = getattr(self, "_aff", None)
        if allst is None:
            allst = self._aff = {}
        st = allst.get(who)
        key = tuple((t.data_ptr(), t._version) for t in (a.fc1.weight, a.fc1.bias, a.fc2.weight, a.fc2.bias))
        if st is None or st["ws"].numel() < need or st["max_B"] < max_B:
            st = allst[who] = dict(ws=torch.empty(int(need), dtype=torch.uint8, device=self.device), max_B=int(max_B), key=None)
        w = _capi.AffinityWeights()
        w.fc1_w, w.fc1_b, w.fc2_w, w.fc2_b = (a.fc1.weight.data_ptr(), a.fc1.bias.data_ptr(), a.fc2.weight.data_ptr(),
                                              a.fc2.bias.data_ptr())
        ready = st["key"] == key
        st["key"] = key
        return st, w, ready

    @torch.no_grad()
    def score_device(self, emb):
        """sigmoid(affinity_score([src | src], [dst | neg])) for the [3B, H] embeddings of a batch -> float32 [2B]:
        the B positive probabilities, then the B negative ones (compute_edge_probabilities' tail, eval mode).  zt_affinity for
        every hidden width it takes (H % 4 == 0, 4 <= H <= 768); torch's MergeLayer for the others."""
        B = emb.shape[0] // 3
        st = self._affinity_state(B)
        if st is None:
            score = self.affinity_score(torch.cat([emb[:B], emb[:B]]), emb[B:]).squeeze(1)
            return score.sigmoid()
        st, w, ready = st
        prob = torch.empty(2 * B, dtype=torch.float32, device=self.device)
        check(lib().zt_affinity(ptr(emb.contiguous()), C.c_int64(B), C.c_int32(emb.shape[1]), C.byref(w), ptr(prob), ptr(st["ws"]),
                                C.c_int64(st["max_B"]), C.c_int32(1 if ready else 0), stream_ptr()), "zt_affinity")
        return prob

    # ------------------------------------------------------------------ read-only queries and ranking
    def _as_device(self, a, dtype):
        """numpy array, list or tensor -> contiguous 1-D+ tensor of ``dtype`` on this model's device"""
        if torch.is_tensor(a):
            return a.to(self.device, dtype).contiguous()
        npd = {torch.int32: np.int32, torch.float64: np.float64}[dtype]
        return torch.from_numpy(np.ascontiguousarray(a, npd)).to(self.device)

    @torch.no_grad()
    def embed_nodes(self, nodes, timestamps, check_status=True):
        """Embeddings of arbitrary nodes at arbitrary times from the model's CURRENT state, read-only: numpy arrays or
        tensors in, a float32 [N, D (n_tppr + 1)] CUDA tensor out.  The T-PPR rows come from ``query_device`` (no update),
        the forward is the eval one (``embed_device`` on the memory table); no message is stored, no memory row, no T-PPR
        dictionary and no ``batch_counter`` changes.  RuntimeError when the model is not in test mode -- messages of
        training batches are pending: run ``update_memory_in_test`` through an eval step first -- or when the native
        pipeline is enabled: its streams and the batches it has queried ahead are not covered by this call."""
        if getattr(self, "_pipe", None) is not None:
            raise RuntimeError("embed_nodes does not cover the native pipeline (its streams, and batches queried ahead, "
                               "whose T-PPR updates are applied already): call enable_pipeline(False) first")
        if not self.test_mode:
            raise RuntimeError("embed_nodes needs the model in test mode: messages of training batches are pending; run an "
                               "eval step (step_device / compute_temporal_embeddings(train=False)) first")
        nodes_d = self._as_device(nodes, torch.int32).reshape(-1)
        ts_d = self._as_device(timestamps, torch.float64).reshape(-1)
        if nodes_d.numel() != ts_d.numel():
            raise ValueError("embed_nodes takes one timestamp per node")
        em = self.embedding_module
        if nodes_d.numel() == 0:
            return torch.empty((0, self.embedding_dimension * (em.n_tppr + 1)), dtype=torch.float32, device=self.device)
        on, oe, od, ow = em.query_device(nodes_d, ts_d, check_status=check_status)
        return em.embed_device(self.memory.memory, nodes_d, on, oe, od, ow, check_status=check_status, memory_obj=self.memory)

    @torch.no_grad()
    def classify_nodes(self, decoder, nodes, timestamps, check_status=True):
        """Probabilities [N] (CUDA) of ``decoder`` (zebra_amd.decoder.MLP) on the embeddings of ``nodes`` at ``timestamps``
        from the model's current state: ``embed_nodes``, then ``decoder.predict``.  Read-only; it refuses what ``embed_nodes``
        refuses."""
        return decoder.predict(self.embed_nodes(nodes, timestamps, check_status=check_status))

    @torch.no_grad()
    def rank_scores(self, emb_q, emb_c, cand_idx=None, check_status=True):
        """prob [Q, C] = sigmoid(affinity_score(emb_q[q], emb_c[cand_idx[q, c]])): one source against many candidates.
        ``cand_idx`` int32 [Q, C] names rows of ``emb_c`` (-1: absent, probability 0) or is None: every query takes all of
        ``emb_c``.  float32 CUDA embeddings of a width zt_affinity_rank takes (H % 4 == 0, 4 <= H <= 4352) go through it
        (csrc/rank.hip); anything else through torch's composition, a chunk of queries at a time."""
        a = self.affinity_score
        Q, H = emb_q.shape
        Nc = emb_c.shape[0]
        C_ = Nc if cand_idx is None else cand_idx.shape[1]
        hip = (emb_q.is_cuda and emb_c.is_cuda and emb_q.dtype == torch.float32 and emb_c.dtype == torch.float32
               and H % 4 == 0 and _capi.RANK_MIN_H <= H <= _capi.RANK_MAX_H)
        if not hip:
            out = torch.zeros((Q, C_), dtype=emb_q.dtype, device=emb_q.device)
            if Q == 0 or C_ == 0:
                return out
            step = max(1, (1 << 24) // max(1, C_ * 2 * H))
            for s in range(0, Q, step):
                q = emb_q[s:s + step]
                if cand_idx is None:
                    ec = emb_c.unsqueeze(0).expand(q.shape[0], Nc, H)
                    live = None
                else:
                    ix = cand_idx[s:s + step].long()
                    if int(ix.max()) >= Nc or int(ix.min()) < -1:
                        raise IndexError("rank_scores: candidate index out of range")
                    live = ix >= 0
                    ec = emb_c[ix.clamp(min=0)]
                x = torch.cat([q.unsqueeze(1).expand(-1, C_, -1), ec], dim=2)
                p = a.fc2(a.act(a.fc1(x))).squeeze(2).sigmoid()
                out[s:s + step] = p if live is None else torch.where(live, p, torch.zeros_like(p))
            return out
        prob = torch.empty((Q, C_), dtype=torch.float32, device=self.device)
        if Q == 0 or C_ == 0:
            return prob
        need = int(lib().zt_affinity_rank_workspace_bytes(C.c_int64(Q), C.c_int64(Nc), C.c_int32(H)))
        ws = getattr(self, "_rank_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._rank_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        w = _capi.AffinityWeights()
        w.fc1_w, w.fc1_b, w.fc2_w, w.fc2_b = (a.fc1.weight.data_ptr(), a.fc1.bias.data_ptr(), a.fc2.weight.data_ptr(),
                                              a.fc2.bias.data_ptr())
        ix = None if cand_idx is None else cand_idx.to(self.device, torch.int32).contiguous()
        check(lib().zt_affinity_rank(ptr(emb_q.contiguous()), C.c_int64(Q), ptr(emb_c.contiguous()), C.c_int64(Nc), ptr(ix),
                                     C.c_int64(C_), C.c_int32(H), C.byref(w), ptr(prob), ptr(ws), stream_ptr()),
              "zt_affinity_rank")
        if check_status and ix is not None:
            st = int(ws[:4].view(torch.int32).item())           # the call's status word: first int32 of the workspace
            if st != 0:
                raise IndexError("zt_affinity_rank: candidate index out of range (status %d)" % st)
        return prob

    @torch.no_grad()
    def rank_candidates(self, sources, timestamps, candidates, check_status=True):
        """prob [Q, C] (CUDA) of ``sources[q]`` interacting with each of its candidates at ``timestamps[q]``, read-only
        (``embed_nodes``): ``candidates`` is [Q, C] (-1: absent, probability 0) or [C], shared by all queries.  Every
        distinct (candidate, time of its query) pair is embedded once."""
        src_d = self._as_device(sources, torch.int32).reshape(-1)
        ts_d = self._as_device(timestamps, torch.float64).reshape(-1)
        cand = self._as_device(candidates, torch.int32)
        Q = src_d.numel()
        if cand.dim() == 1:
            cand = cand.unsqueeze(0).expand(Q, -1)
        if cand.dim() != 2 or cand.shape[0] != Q or ts_d.numel() != Q:
            raise ValueError("rank_candidates takes sources [Q], timestamps [Q] and candidates [Q, C] or [C]")
        emb_q, emb_c, cand_idx = self._embed_candidates(src_d, ts_d, cand.contiguous(), check_status)
        return self.rank_scores(emb_q, emb_c, cand_idx, check_status=check_status)

    def _embed_candidates(self, src_d, ts_d, cand, check_status):
        """(emb_q, emb_c, cand_idx) of sources [Q] at times [Q] and their candidates [Q, C] (-1: absent): every distinct
        (candidate, time of its query) pair is embedded once, cand_idx names its row of emb_c."""
        emb_q = self.embed_nodes(src_d, ts_d, check_status=check_status)
        live = cand >= 0
        t_of = ts_d.unsqueeze(1).expand_as(cand)
        pairs = torch.stack([cand[live].to(torch.float64), t_of[live]])          # (node ids are exact in float64)
        uniq, inv = torch.unique(pairs, dim=1, return_inverse=True)
        emb_c = self.embed_nodes(uniq[0].to(torch.int32), uniq[1].contiguous(), check_status=check_status)
        cand_idx = torch.full(cand.shape, -1, dtype=torch.int32, device=self.device)
        cand_idx[live] = inv.to(torch.int32)
        return emb_q, emb_c, cand_idx

    # ---- per-query exclusions: absent bits (include/zebra_amd.h, zt_affinity_topk_masked) ----
    def _exclude_lists(self, src_d, ts_d, exclude):
        """(handle, ids, begin, len) of the per-query id lists ``exclude`` names (``absent_bits``): ranges of the finder's own
        neighbour array (ids None: nothing is copied), or of the caller's array (handle None)."""
        from .tppr import NeighborFinder
        Q = src_d.numel()
        if isinstance(exclude, str):
            if exclude != "seen":
                raise ValueError("exclude is \"seen\", a NeighborFinder or (ptr [Q + 1], ids)")
            exclude = self.neighbor_finder
            if exclude is None:
                raise ValueError("exclude=\"seen\" needs the model's neighbor_finder; pass a NeighborFinder")
        if isinstance(exclude, NeighborFinder):
            begin, length = exclude.seen_ranges_device(src_d, ts_d)
            return exclude._h, None, begin, length
        if not (isinstance(exclude, (tuple, list)) and len(exclude) == 2):
            raise ValueError("exclude is \"seen\", a NeighborFinder or (ptr [Q + 1], ids)")
        lp = exclude[0] if torch.is_tensor(exclude[0]) else torch.from_numpy(np.ascontiguousarray(exclude[0], np.int64))
        lp = lp.to(self.device, torch.int64).reshape(-1)
        ids = self._as_device(exclude[1], torch.int32).reshape(-1)
        if lp.numel() != Q + 1:
            raise ValueError("exclude=(ptr, ids): ptr holds Q + 1 offsets into ids")
        if Q > 0:                                                     # (the kernel trusts the caller's ranges: one host read)
            bad = (lp[1:] < lp[:-1]).any() | (lp[0] < 0) | (lp[-1] > ids.numel())
            if bool(bad):
                raise ValueError("exclude=(ptr, ids): ptr must ascend from >= 0 to <= len(ids)")
        if ids.numel() == 0:
            ids = torch.zeros(1, dtype=torch.int32, device=self.device)        # (an address to hand over; never read)
        return None, ids, lp[:-1].contiguous(), (lp[1:] - lp[:-1]).contiguous()

    def _mark_absent(self, lists, Q, id_lo=None, n_cols=None, candidates=None):
        """zt_exclude_mark: int32 [Q, ceil(C / 32)] absent bits of the lists over a range of ids or a candidate list"""
        handle, ids, begin, length = lists
        if candidates is None:
            if id_lo is None or n_cols is None:
                raise ValueError("absent_bits takes candidates, or id_lo and n_cols for the ids id_lo .. id_lo + n_cols - 1")
            C_, srt, col, stride = int(n_cols), None, None, 0
        else:
            cand = candidates
            if cand.dim() not in (1, 2) or (cand.dim() == 2 and cand.shape[0] != Q):
                raise ValueError("absent_bits takes candidates [Q, C] or [C]")
            C_ = cand.shape[-1]
            srt, order = torch.sort(cand, dim=-1)
            srt, col = srt.contiguous(), order.to(torch.int32).contiguous()
            stride = C_ if cand.dim() == 2 else 0
            id_lo = 0
        if C_ < 0:
            raise ValueError("absent_bits: n_cols must not be negative")
        W = (C_ + 31) // 32
        absent = torch.empty((Q, W), dtype=torch.int32, device=self.device)
        if Q == 0 or W == 0:
            return absent
        check(lib().zt_exclude_mark(handle, ptr(ids), ptr(begin), ptr(length), C.c_int64(Q), C.c_int64(int(id_lo)), ptr(srt),
                                    ptr(col), C.c_int64(stride), C.c_int64(C_), ptr(absent), C.c_int64(W), stream_ptr()),
              "zt_exclude_mark")
        return absent

    @torch.no_grad()
    def absent_bits(self, sources, timestamps, exclude, *, id_lo=None, n_cols=None, candidates=None):
        """int32 [Q, ceil(C / 32)] on the device, the absent bits ``topk_scores(absent=...)`` takes: bit c & 31 of word c >> 5
        of row q is set where column c of the pool is excluded for ``sources[q]``.  ``exclude``: "seen" -- the partners of the
        source strictly before ``timestamps[q]`` in ``self.neighbor_finder`` (ValueError if the model has none) --, a
        NeighborFinder to take them from, or (ptr [Q + 1] int64, ids int32): the caller's own lists, ids[ptr[q]:ptr[q + 1]]
        for query q.  Lists may hold duplicates and ids outside the pool.  The pool: ``candidates`` [C] (shared) or [Q, C]
        (-1: absent entries, never matched; every column that holds an excluded id is set), or the ids ``id_lo`` ..
        ``id_lo + n_cols - 1`` in order.  The lists are built and marked on the device (zt_csr_seen_ranges, zt_exclude_mark);
        a "seen" list is a range of the finder's own array, never copied.  IndexError for a source outside the finder."""
        src_d = self._as_device(sources, torch.int32).reshape(-1)
        Q = src_d.numel()
        ts_d = self._as_device(timestamps, torch.float64).reshape(-1)
        if ts_d.numel() == 1 and Q != 1:
            ts_d = ts_d.expand(Q).contiguous()
        if ts_d.numel() != Q:
            raise ValueError("absent_bits takes sources [Q] and timestamps [Q] or a scalar")
        cand = None if candidates is None else self._as_device(candidates, torch.int32)
        return self._mark_absent(self._exclude_lists(src_d, ts_d, exclude), Q, id_lo, n_cols, cand)

    @torch.no_grad()
    def topk_scores(self, emb_q, emb_c, k, cand_idx=None, skip=None, idx_base=0, out=None, check_status=True,
                    workspace_bytes=None, absent=None):
        """(idx [Q, k] int32, prob [Q, k] float32): for every query the ``k`` present candidates of ``rank_scores`` with the
        largest probability, descending, equal probabilities in ascending index; slots beyond the present candidates read -1
        and 0.  ``idx`` is ``idx_base`` + the column in [0, C).  Present: ``cand_idx`` (if given) is >= 0, the probability is not
        NaN -- nor any element of the candidate's embedding -- and ``idx_base`` + column differs from ``skip[q]`` (int32 [Q],
        -1: none).  ``out=(idx, prob)``: the entries already
        there (-1: empty) compete with this call's candidates and the result is written into them -- a pool given in pieces, with
        ``idx_base`` set accordingly, gives the bits of one call.  Where ``rank_scores`` would call zt_affinity_rank and
        k <= 256 this is zt_affinity_topk (csrc/rank_topk.hip): prob[Q, C] is never written and the workspace does not grow
        with the pool (``workspace_bytes``: its size, zt_affinity_topk_workspace_bytes by default).  Anything else computes
        ``rank_scores`` a chunk of queries at a time and selects by stable sorts with the same rule.
        ``absent``: int32 (or uint32) [Q, W >= ceil(C / 32)] absent bits (``absent_bits``) -- a set bit c & 31 of word c >> 5 of
        row q takes the LOCAL column c of this call out of query q's candidates; the HIP path is then zt_affinity_topk_masked,
        and the torch path honours the same bits."""
        a = self.affinity_score
        Q, H = emb_q.shape
        Nc = emb_c.shape[0]
        C_ = Nc if cand_idx is None else cand_idx.shape[1]
        k = int(k)
        if k <= 0:
            raise ValueError("topk_scores: k must be positive")
        if idx_base < 0 or idx_base + C_ > 0x7fffffff:
            raise ValueError("topk_scores: idx_base + C exceeds the int32 indices of the result")
        dev = emb_q.device
        if out is not None:
            top_idx, top_prob = out
            if (top_idx.shape != (Q, k) or top_prob.shape != (Q, k) or top_idx.dtype != torch.int32 or top_prob.dtype != torch.float32
                    or top_idx.device != dev or top_prob.device != dev or not top_idx.is_contiguous() or not top_prob.is_contiguous()):
                raise ValueError("topk_scores: out is (idx [Q, k] int32, prob [Q, k] float32), contiguous, on the embeddings' device")
        if absent is not None:
            if absent.dtype != torch.int32:
                if absent.dtype != getattr(torch, "uint32", None):
                    raise ValueError("topk_scores: absent is int32 or uint32 [Q, W]")
                absent = absent.view(torch.int32)
            if absent.dim() != 2 or absent.shape[0] != Q or absent.shape[1] < (C_ + 31) // 32:
                raise ValueError("topk_scores: absent is [Q, W] with W >= ceil(C / 32)")
            absent = absent.to(dev).contiguous()
        hip = (emb_q.is_cuda and emb_c.is_cuda and emb_q.dtype == torch.float32 and emb_c.dtype == torch.float32
               and H % 4 == 0 and _capi.RANK_MIN_H <= H <= _capi.RANK_MAX_H and k <= _capi.TOPK_MAX_K)
        if not hip:
            if out is None:
                top_idx = torch.full((Q, k), -1, dtype=torch.int32, device=dev)
                top_prob = torch.zeros((Q, k), dtype=torch.float32, device=dev)
            if Q == 0 or C_ == 0:
                return top_idx, top_prob
            col = torch.arange(C_, device=dev, dtype=torch.int64) + int(idx_base)
            step = max(1, (1 << 24) // max(1, C_))
            for s in range(0, Q, step):
                ix = None if cand_idx is None else cand_idx[s:s + step]
                p = self.rank_scores(emb_q[s:s + step], emb_c, ix, check_status=check_status).to(torch.float32)
                live = ~torch.isnan(p)
                nan_row = torch.isnan(emb_c).any(dim=1)          # (the kernels' relu drops a NaN: such a row is a NaN candidate)
                if ix is None:
                    live &= ~nan_row.unsqueeze(0)
                else:
                    ixd = ix.to(dev).long()
                    live &= (ixd >= 0) & (ixd < Nc)
                    live &= ~nan_row[ixd.clamp(0, max(Nc - 1, 0))]
                if skip is not None:
                    live &= col.unsqueeze(0) != skip[s:s + step].to(dev, torch.int64).unsqueeze(1)
                if absent is not None:
                    live &= ~absent_columns(absent[s:s + step], C_)
                # this call's candidates behind the incoming list; absent entries sort last (probabilities are >= 0)
                n = p.shape[0]
                all_i = torch.cat([top_idx[s:s + step].to(torch.int64), col.unsqueeze(0).expand(n, -1)], dim=1)
                all_p = torch.cat([top_prob[s:s + step], p], dim=1)
                all_live = torch.cat([top_idx[s:s + step] >= 0, live], dim=1)
                all_p = torch.where(all_live, all_p, torch.full_like(all_p, -1.0))
                o1 = torch.sort(all_i, dim=1, stable=True).indices               # ascending index, then a stable sort by
                o2 = torch.sort(all_p.gather(1, o1), dim=1, descending=True, stable=True).indices[:, :k]    # probability
                sel = o1.gather(1, o2)
                got = all_live.gather(1, sel)
                kk = sel.shape[1]
                top_idx[s:s + step, :kk] = torch.where(got, all_i.gather(1, sel), torch.full_like(sel, -1)).to(torch.int32)
                top_prob[s:s + step, :kk] = torch.where(got, all_p.gather(1, sel), torch.zeros_like(all_p[:, :kk]))
            return top_idx, top_prob
        accumulate = out is not None
        if not accumulate:
            top_idx = torch.empty((Q, k), dtype=torch.int32, device=self.device)
            top_prob = torch.empty((Q, k), dtype=torch.float32, device=self.device)
        if Q == 0:
            return top_idx, top_prob
        need = int(lib().zt_affinity_topk_workspace_bytes(C.c_int64(Q), C.c_int64(Nc), C.c_int32(H), C.c_int32(k)))
        if workspace_bytes is not None:
            need = int(workspace_bytes)
        ws = getattr(self, "_topk_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._topk_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        w = _capi.AffinityWeights()
        w.fc1_w, w.fc1_b, w.fc2_w, w.fc2_b = (a.fc1.weight.data_ptr(), a.fc1.bias.data_ptr(), a.fc2.weight.data_ptr(),
                                              a.fc2.bias.data_ptr())
        ix = None if cand_idx is None else cand_idx.to(self.device, torch.int32).contiguous()
        sk = None if skip is None else skip.to(self.device, torch.int32).contiguous()
        if sk is not None and sk.numel() != Q:
            raise ValueError("topk_scores: skip holds one column per query")
        emb_c = emb_c.contiguous()
        if C_ == 0:                        # an empty tensor has no address: one to hand over, never read (C = 0: -1 and 0, or
            if Nc == 0:                    # the incoming list left alone; found by test_topk_exact_gpu.py, orders-*-K1-C0)
                emb_c = torch.zeros((1, H), dtype=torch.float32, device=self.device)
            if ix is not None:
                ix = torch.zeros(1, dtype=torch.int32, device=self.device)
        args = (ptr(emb_q.contiguous()), C.c_int64(Q), ptr(emb_c), C.c_int64(Nc), ptr(ix), C.c_int64(C_), C.c_int32(H),
                C.byref(w), C.c_int32(k), ptr(sk), C.c_int64(int(idx_base)), C.c_int32(1 if accumulate else 0), ptr(top_idx),
                ptr(top_prob), ptr(ws), C.c_int64(need))
        if absent is None or absent.shape[1] == 0:                     # (C = 0: no words, and no address to hand over)
            check(lib().zt_affinity_topk(*args, stream_ptr()), "zt_affinity_topk")
        else:
            check(lib().zt_affinity_topk_masked(*args, ptr(absent), C.c_int64(absent.shape[1]), stream_ptr()),
                  "zt_affinity_topk_masked")
        if check_status and ix is not None and C_ > 0:
            st = int(ws[:4].view(torch.int32).item())           # the call's status word: first int32 of the workspace
            if st != 0:
                raise IndexError("zt_affinity_topk: candidate index out of range (status %d)" % st)
        return top_idx, top_prob

    @torch.no_grad()
    def recommend(self, sources, timestamps, k, candidates=None, exclude_self=True, pool_chunk=65536, exclude=None):
        """(nodes [Q, k] int32, prob [Q, k] float32): the ``k`` likeliest partners of every source among ``candidates``, -1 and 0
        in empty slots; read-only, and raises where ``embed_nodes`` raises.
        ``candidates=None``: every node id 1 .. n_nodes - 1 (0 is the padding id), without the source's own id under
        ``exclude_self``; a 1-D list: a pool shared by all queries (-1: absent).  Both are embedded ``pool_chunk`` rows at a time
        and each chunk goes through ``topk_scores`` with accumulate, so memory does not depend on the pool; ``timestamps`` is
        then a scalar or all equal (ValueError otherwise: a candidate's embedding depends on the query's time).
        ``candidates`` [Q, C] (-1: absent) takes per-query times: ``rank_candidates``' de-duplication, then ``topk_scores``.
        ``exclude`` (None: nothing more is left out): per-query lists of ids that must not come back, as ``absent_bits`` takes
        them -- "seen": the partners each source has met strictly before its query time, from ``self.neighbor_finder``; a
        NeighborFinder; or (ptr [Q + 1], ids).  Every pool chunk gets its absent bits on the device (Q * ceil(pool_chunk / 32)
        words: memory still does not grow with the pool) and the fused top-K leaves those columns out, so k results come back
        wherever k candidates remain, whatever the source's degree.  ``exclude_self`` works beside it."""
        src_d = self._as_device(sources, torch.int32).reshape(-1)
        Q = src_d.numel()
        ts_d = self._as_device(timestamps, torch.float64).reshape(-1)
        if ts_d.numel() == 1 and Q != 1:
            ts_d = ts_d.expand(Q).contiguous()
        k = int(k)
        if ts_d.numel() != Q or k <= 0 or int(pool_chunk) <= 0:
            raise ValueError("recommend takes sources [Q], timestamps [Q] or a scalar, k > 0 and pool_chunk > 0")
        cand = None if candidates is None else self._as_device(candidates, torch.int32)
        if exclude is not None:                                      # (refuses where embed_nodes does, before any device work)
            self.embed_nodes(src_d[:0], ts_d[:0])
            lists = self._exclude_lists(src_d, ts_d, exclude)
        if cand is not None and cand.dim() == 2:
            if cand.shape[0] != Q:
                raise ValueError("recommend takes candidates [Q, C] or [C]")
            emb_q, emb_c, cand_idx = self._embed_candidates(src_d, ts_d, cand.contiguous(), True)
            absent = None if exclude is None else self._mark_absent(lists, Q, candidates=cand)
            idx, prob = self.topk_scores(emb_q, emb_c, k, cand_idx=cand_idx, absent=absent)
            nodes = torch.where(idx >= 0, cand.gather(1, idx.clamp(min=0).long()), torch.full_like(idx, -1))
            return nodes, prob
        if cand is not None and cand.dim() != 1:
            raise ValueError("recommend takes candidates [Q, C] or [C]")
        if Q > 0 and bool((ts_d != ts_d[0]).any()):
            raise ValueError("recommend: a shared pool needs one query time (a scalar, or all timestamps equal): a candidate's "
                             "embedding depends on it; give candidates [Q, C] for per-query times")
        emb_q = self.embed_nodes(src_d, ts_d)
        n_pool = self.n_nodes - 1 if cand is None else cand.numel()
        idx = torch.full((Q, k), -1, dtype=torch.int32, device=self.device)
        prob = torch.zeros((Q, k), dtype=torch.float32, device=self.device)
        if Q == 0 or n_pool <= 0:
            return idx, prob
        skip = (src_d - 1) if (cand is None and exclude_self) else None      # node id v is column v - 1 of the pool 1 .. n - 1
        for s in range(0, n_pool, int(pool_chunk)):
            e = min(n_pool, s + int(pool_chunk))
            ids = torch.arange(s + 1, e + 1, dtype=torch.int32, device=self.device) if cand is None else cand[s:e]
            emb_c = self.embed_nodes(ids.clamp(min=0), ts_d[:1].expand(e - s).contiguous())
            cix = None
            if cand is not None and bool((ids < 0).any()):                 # absent entries of a shared list: through indices
                cix = torch.where(ids >= 0, torch.arange(e - s, dtype=torch.int32, device=self.device),
                                  torch.full_like(ids, -1)).unsqueeze(0).expand(Q, -1).contiguous()
            absent = None
            if exclude is not None:
                absent = (self._mark_absent(lists, Q, id_lo=s + 1, n_cols=e - s) if cand is None
                          else self._mark_absent(lists, Q, candidates=ids))
            self.topk_scores(emb_q, emb_c, k, cand_idx=cix, skip=skip, idx_base=s, out=(idx, prob), absent=absent)
        if cand is None:
            nodes = torch.where(idx >= 0, idx + 1, idx)
        else:
            nodes = torch.where(idx >= 0, cand[idx.clamp(min=0).long()], torch.full_like(idx, -1))
        return nodes, prob

    @torch.no_grad()
    def count_scores(self, emb_q, emb_c, thr, skip=None, idx_base=0, out=None, absent=None, workspace_bytes=None):
        """(above [Q] int32, equal [Q] int32): for every query the number of present candidates of ``rank_scores(emb_q, emb_c)``
        whose probability is above ``thr[q]`` (float32 [Q]) and the number equal to it -- IEEE compares: a NaN threshold counts
        nothing.  Present: ``topk_scores``' rule for a shared pool -- the probability is not NaN, nor any element of the
        candidate's embedding; ``idx_base`` + column differs from every entry of ``skip`` (int32 [Q] or [Q, n], n <= 4, -1:
        none); the column's bit of ``absent`` (int32 or uint32 [Q, W >= ceil(C / 32)], ``absent_bits``) is clear.
        ``out=(above, equal)``: the counts are ADDED to what is there -- a pool given in pieces, in any order, with ``idx_base``
        and local bits per piece, gives the numbers of one call.  Where ``rank_scores`` would call zt_affinity_rank this is
        zt_affinity_count (csrc/rank_count.hip): prob[Q, C] is never written and the workspace does not grow with the pool
        (``workspace_bytes``: its size, zt_affinity_count_workspace_bytes by default).  Anything else computes ``rank_scores`` a
        chunk of queries at a time and counts under the same rule."""
        a = self.affinity_score
        Q, H = emb_q.shape
        Nc = emb_c.shape[0]
        dev = emb_q.device
        if idx_base < 0 or idx_base + Nc > 0x7fffffff:
            raise ValueError("count_scores: idx_base + C exceeds int32 columns")
        if thr.dim() != 1 or thr.numel() != Q:
            raise ValueError("count_scores: thr holds one threshold per query")
        thr = thr.to(dev, torch.float32).contiguous()
        if out is not None:
            above, equal = out
            for t in (above, equal):
                if t.shape != (Q,) or t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
                    raise ValueError("count_scores: out is (above [Q] int32, equal [Q] int32), contiguous, on the embeddings' device")
        if skip is not None:
            skip = skip.to(dev, torch.int32)
            if skip.dim() == 1:
                skip = skip.unsqueeze(1)
            if skip.dim() != 2 or skip.shape[0] != Q or skip.shape[1] > _capi.COUNT_MAX_SKIP:
                raise ValueError("count_scores: skip is [Q] or [Q, n] with n <= %d" % _capi.COUNT_MAX_SKIP)
            skip = None if skip.shape[1] == 0 else skip.contiguous()
        if absent is not None:
            if absent.dtype != torch.int32:
                if absent.dtype != getattr(torch, "uint32", None):
                    raise ValueError("count_scores: absent is int32 or uint32 [Q, W]")
                absent = absent.view(torch.int32)
            if absent.dim() != 2 or absent.shape[0] != Q or absent.shape[1] < (Nc + 31) // 32:
                raise ValueError("count_scores: absent is [Q, W] with W >= ceil(C / 32)")
            absent = absent.to(dev).contiguous()
        if out is None:
            above = torch.zeros(Q, dtype=torch.int32, device=dev)
            equal = torch.zeros(Q, dtype=torch.int32, device=dev)
        hip = (emb_q.is_cuda and emb_c.is_cuda and emb_q.dtype == torch.float32 and emb_c.dtype == torch.float32
               and H % 4 == 0 and _capi.RANK_MIN_H <= H <= _capi.RANK_MAX_H)
        if Q == 0 or Nc == 0:
            return above, equal
        if not hip:
            col = torch.arange(Nc, device=dev, dtype=torch.int64) + int(idx_base)
            nan_row = torch.isnan(emb_c).any(dim=1)              # (the kernels' relu drops a NaN: such a row is a NaN candidate)
            step = max(1, (1 << 24) // max(1, Nc))
            for s in range(0, Q, step):
                p = self.rank_scores(emb_q[s:s + step], emb_c).to(torch.float32)
                live = ~torch.isnan(p) & ~nan_row.unsqueeze(0)
                if skip is not None:
                    for j in range(skip.shape[1]):
                        live &= col.unsqueeze(0) != skip[s:s + step, j].to(torch.int64).unsqueeze(1)
                if absent is not None:
                    live &= ~absent_columns(absent[s:s + step], Nc)
                t = thr[s:s + step].unsqueeze(1)
                above[s:s + step] += (live & (p > t)).sum(dim=1).to(torch.int32)
                equal[s:s + step] += (live & (p == t)).sum(dim=1).to(torch.int32)
            return above, equal
        need = int(lib().zt_affinity_count_workspace_bytes(C.c_int64(Q), C.c_int64(Nc), C.c_int32(H)))
        if workspace_bytes is not None:
            need = int(workspace_bytes)
        ws = getattr(self, "_count_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._count_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        w = _capi.AffinityWeights()
        w.fc1_w, w.fc1_b, w.fc2_w, w.fc2_b = (a.fc1.weight.data_ptr(), a.fc1.bias.data_ptr(), a.fc2.weight.data_ptr(),
                                              a.fc2.bias.data_ptr())
        n_skip = 0 if skip is None else skip.shape[1]
        if out is None:                                              # (a fresh call: the library zeroes what it adds to)
            above = torch.empty(Q, dtype=torch.int32, device=self.device)
            equal = torch.empty(Q, dtype=torch.int32, device=self.device)
        check(lib().zt_affinity_count(ptr(emb_q.contiguous()), C.c_int64(Q), ptr(emb_c.contiguous()), C.c_int64(Nc), C.c_int32(H),
                                      C.byref(w), ptr(thr), ptr(skip), C.c_int32(n_skip), C.c_int64(int(idx_base)),
                                      C.c_int32(0 if out is None else 1), ptr(above), ptr(equal), ptr(ws), C.c_int64(need),
                                      ptr(absent),
                                      C.c_int64(0 if absent is None else absent.shape[1]), stream_ptr()), "zt_affinity_count")
        return above, equal

    @staticmethod
    def _pack_absent(gone):
        """int32 [Q, ceil(C / 32)] absent bits of a bool [Q, C] (bit c & 31 of word c >> 5: ``absent_columns``' inverse)"""
        Q, C_ = gone.shape
        W = (C_ + 31) // 32
        padded = torch.zeros((Q, W * 32), dtype=torch.int64, device=gone.device)
        padded[:, :C_] = gone
        words = (padded.view(Q, W, 32) << torch.arange(32, dtype=torch.int64, device=gone.device)).sum(dim=2)
        return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)

    @torch.no_grad()
    def rank_of(self, sources, timestamps, targets, candidates=None, exclude_self=True, pool_chunk=65536, exclude=None,
                exclude_timestamps=None, counts=False):
        """(rank [Q] float64, prob [Q] float32): where ``targets[q]`` stands among the candidates ``recommend`` would rank for
        ``sources[q]`` at ``timestamps[q]`` -- rank = 1 + (present candidates with a larger probability) + 0.5 (present
        candidates with an equal one), the mean of the optimistic and the pessimistic rank; ``prob`` is the target's own
        probability, ``rank_scores`` of (source, target) both embedded at the query time.  ``counts=True`` returns (above
        [Q] int32, equal [Q] int32, prob) instead.  The target is never counted against itself; a target < 0 gives rank 0
        (counts 0, probability 0).  Read-only; raises where ``embed_nodes`` raises.
        ``candidates=None`` (every node id 1 .. n_nodes - 1, without the source's own id under ``exclude_self``) or a 1-D list
        (-1: absent; duplicates allowed): ``recommend``'s shared-pool walk -- the pool is embedded ``pool_chunk`` rows at a time
        and every chunk goes through ``count_scores`` with accumulate, so prob[Q, pool] never exists and memory does not depend
        on the pool; ``timestamps`` is then a scalar or all equal (``recommend``'s ValueError otherwise).  ``candidates``
        [Q, C] (-1: absent) takes per-query times: ``rank_candidates`` on [target | C], then ``evaluation.rank_metrics``.
        ``exclude``: as ``recommend`` takes it -- "seen", a NeighborFinder or (ptr [Q + 1], ids) -- with the "seen" lists cut at
        ``exclude_timestamps`` [Q] (default: the query times).  An excluded id that is the target still is the target: it has
        its rank among the others."""
        src_d = self._as_device(sources, torch.int32).reshape(-1)
        Q = src_d.numel()
        ts_d = self._as_device(timestamps, torch.float64).reshape(-1)
        if ts_d.numel() == 1 and Q != 1:
            ts_d = ts_d.expand(Q).contiguous()
        tgt_d = self._as_device(targets, torch.int32).reshape(-1)
        if ts_d.numel() != Q or tgt_d.numel() != Q or int(pool_chunk) <= 0:
            raise ValueError("rank_of takes sources [Q], timestamps [Q] or a scalar, targets [Q] and pool_chunk > 0")
        ets_d = ts_d
        if exclude_timestamps is not None:
            ets_d = self._as_device(exclude_timestamps, torch.float64).reshape(-1)
            if ets_d.numel() != Q:
                raise ValueError("rank_of takes exclude_timestamps [Q]")
        cand = None if candidates is None else self._as_device(candidates, torch.int32)
        if cand is not None and (cand.dim() not in (1, 2) or (cand.dim() == 2 and cand.shape[0] != Q)):
            raise ValueError("rank_of takes candidates [Q, C] or [C]")
        self.embed_nodes(src_d[:0], ts_d[:0])                        # (refuses where embed_nodes does, before any device work)
        lists = None if exclude is None else self._exclude_lists(src_d, ets_d, exclude)
        has = tgt_d >= 0
        if cand is not None and cand.dim() == 2:
            from .evaluation import rank_metrics
            gone = (cand == tgt_d.unsqueeze(1)) | (cand < 0)
            if lists is not None:
                gone |= absent_columns(self._mark_absent(lists, Q, candidates=cand.contiguous()), cand.shape[1])
            table = torch.cat([tgt_d.unsqueeze(1), torch.where(gone, torch.full_like(cand, -1), cand)], dim=1).contiguous()
            p = self.rank_candidates(src_d, ts_d, table).float()
            prob = p[:, 0].contiguous()
            if counts:
                live = (table[:, 1:] >= 0) & has.unsqueeze(1)
                above = (live & (p[:, 1:] > p[:, :1])).sum(dim=1).to(torch.int32)
                equal = (live & (p[:, 1:] == p[:, :1])).sum(dim=1).to(torch.int32)
                return above, equal, prob
            return rank_metrics(p, table, ranks=True)[1].to(torch.float64), prob
        if Q > 0 and bool((ts_d != ts_d[0]).any()):
            raise ValueError("recommend: a shared pool needs one query time (a scalar, or all timestamps equal): a candidate's "
                             "embedding depends on it; give candidates [Q, C] for per-query times")
        emb_q = self.embed_nodes(src_d, ts_d)
        # the thresholds: rank_scores of (source, target), the target embedded at the query time, through cand_idx [Q, 1]
        prob = torch.zeros(Q, dtype=torch.float32, device=self.device)
        if bool(has.any()):
            uniq, inv = torch.unique(tgt_d[has], return_inverse=True)
            emb_t = self.embed_nodes(uniq, ts_d[:1].expand(uniq.numel()).contiguous())
            tix = torch.full((Q, 1), -1, dtype=torch.int32, device=self.device)
            tix[has, 0] = inv.to(torch.int32)
            prob = self.rank_scores(emb_q, emb_t, tix).float()[:, 0].contiguous()
        thr = torch.where(has, prob, torch.full_like(prob, float("nan")))
        above = torch.zeros(Q, dtype=torch.int32, device=self.device)
        equal = torch.zeros(Q, dtype=torch.int32, device=self.device)
        n_pool = self.n_nodes - 1 if cand is None else cand.numel()
        skip = None
        if cand is None:                                             # node id v is column v - 1 of the pool 1 .. n - 1
            skip = torch.stack([torch.where(has, tgt_d - 1, torch.full_like(tgt_d, -1)),
                                (src_d - 1) if exclude_self else torch.full_like(src_d, -1)], dim=1).contiguous()
        for s in range(0, max(n_pool, 0) if Q > 0 else 0, int(pool_chunk)):
            e = min(n_pool, s + int(pool_chunk))
            ids = torch.arange(s + 1, e + 1, dtype=torch.int32, device=self.device) if cand is None else cand[s:e]
            emb_c = self.embed_nodes(ids.clamp(min=0), ts_d[:1].expand(e - s).contiguous())
            absent = None
            if cand is not None:                                     # the target's columns and the list's -1 entries: bits
                absent = self._pack_absent((ids.unsqueeze(0) == tgt_d.unsqueeze(1)) | (ids < 0).unsqueeze(0))
            if lists is not None:
                bits = (self._mark_absent(lists, Q, id_lo=s + 1, n_cols=e - s) if cand is None
                        else self._mark_absent(lists, Q, candidates=ids.contiguous()))
                absent = bits if absent is None else absent | bits
            self.count_scores(emb_q, emb_c, thr, skip=skip, idx_base=s, out=(above, equal), absent=absent)
        if counts:
            return above, equal, prob
        rank = torch.where(has & ~torch.isnan(prob), 1.0 + above.to(torch.float64) + 0.5 * equal.to(torch.float64),
                           torch.zeros(Q, dtype=torch.float64, device=self.device))
        return rank, prob

    def _score_pairs(self, s, dd, n):
        """The scorer as torch composes it (tgn_model.py:185-188): (pos [B, 1], neg [B, 1]) under autograd."""
        n_samples = s.shape[0]
        score = self.affinity_score(torch.cat([s, s], dim=0), torch.cat([dd, n])).squeeze(dim=0)
        return score[:n_samples].sigmoid(), score[n_samples:].sigmoid()

    def score_train(self, emb):
        """(pos [B, 1], neg [B, 1]) = sigmoid(affinity_score([src | src], [dst | neg])) for the [3B, H] embeddings
        [src | dst | neg] of a training batch, differentiable: csrc/scoring_train.hip through _HipLinkScore where
        link_score_plan says so, else torch's composition."""
        B = emb.shape[0] // 3
        a = self.affinity_score
        if link_score_plan(emb.device.type, emb.dtype, emb.shape[1], getattr(self, "fused_scoring", True)) == "hip":
            prob = _HipLinkScore.apply(emb, a.fc1.weight, a.fc1.bias, a.fc2.weight, a.fc2.bias)
            return prob[:B].unsqueeze(1), prob[B:].unsqueeze(1)
        return self._score_pairs(emb[:B], emb[B:2 * B], emb[2 * B:])

    def score_many_train(self, emb_q, emb_c, cand_idx=None):
        """logits [Q, C] = affinity_score(emb_q[q], emb_c[cand_idx[q, c]]) before the sigmoid, differentiable: one source
        against many candidates in a TRAINING step.  ``cand_idx`` int32 [Q, C] names rows of ``emb_c`` (-1: absent, the logit
        is -inf and takes no gradient; IndexError for anything else outside [0, Nc)) or is None: every query takes all of
        ``emb_c``.  csrc/rank_train.hip through _HipRankScore where rank_score_plan says so -- no [Q, C, H] tensor exists,
        forward or backward -- else torch's composition under autograd, a chunk of queries at a time as in rank_scores."""
        a = self.affinity_score
        Q, H = emb_q.shape
        Nc = emb_c.shape[0]
        C_ = Nc if cand_idx is None else cand_idx.shape[1]
        if (rank_score_plan(emb_q.device.type, emb_q.dtype, H, getattr(self, "fused_scoring", True)) == "hip"
                and emb_c.is_cuda and emb_c.dtype == torch.float32):
            with torch.cuda.device(emb_q.device):
                return _HipRankScore.apply(emb_q, emb_c, cand_idx, a.fc1.weight, a.fc1.bias, a.fc2.weight, a.fc2.bias)
        if Q == 0 or C_ == 0:
            return torch.zeros((Q, C_), dtype=emb_q.dtype, device=emb_q.device)
        ix = None
        if cand_idx is not None:
            ix = cand_idx.to(emb_q.device).long()
            if int(ix.max()) >= Nc or int(ix.min()) < -1:
                raise IndexError("score_many_train: candidate index out of range")
        out = []
        step = max(1, (1 << 24) // max(1, C_ * 2 * H))
        for s in range(0, Q, step):
            q = emb_q[s:s + step]
            ec = emb_c.unsqueeze(0).expand(q.shape[0], Nc, H) if ix is None else emb_c[ix[s:s + step].clamp(min=0)]
            x = torch.cat([q.unsqueeze(1).expand(-1, C_, -1), ec], dim=2)
            lg = a.fc2(a.act(a.fc1(x))).squeeze(2)
            if ix is not None:
                lg = lg.masked_fill(ix[s:s + step] < 0, float("-inf"))
            out.append(lg)
        return torch.cat(out)

    def enable_scoring(self, on=True):
        """With the native pipeline: every whole-batch step also scores its 2B pairs behind its aggregation
        (zt_pipeline_set_scoring); ``last_prob()`` returns the last step's probabilities.  ValueError where the hidden width
        has no HIP scorer (H % 4 != 0 or H > 768): the native step has no torch fallback."""
        self._score_on = bool(on)
        if not on:
            self._met_on = False                         # (zt_pipeline_set_scoring with NULL weights turns the tail off too)
        self._pipe_scoring_sync(force=True)

    def last_prob(self):
        """float32 [2B] view of the last scored step's probabilities (B positive pairs, then B negative ones), valid on
        the caller's current stream; the buffer is reused two steps later."""
        out, B = C.c_void_p(), C.c_int64()
        check(lib().zt_pipeline_last_scores(self._pipe, stream_ptr(), C.byref(out), C.byref(B)), "zt_pipeline_last_scores")
        off = (out.value - self._prob_buf.data_ptr()) // 4
        return self._prob_buf[off: off + 2 * B.value]

    def enable_metrics(self, on=True, per_batch=0):
        """With the native pipeline and ``enable_scoring()``: every scored step is followed by the link-metrics kernel on its
        2B probabilities (zt_pipeline_set_metrics; on the pipeline's message stream, off the main stream's chain), which adds
        the batch's (AP, AUC, accuracy) to a float64 [3] accumulator this model owns and, for ``per_batch`` > 0, writes them to
        row i of a [per_batch, 3] table, i counting the batches since this call.  ``metrics()`` returns them.  RuntimeError
        without a pipeline or without scoring; ValueError where the library refuses (``max_batch`` beyond 16384 pairs, an
        exchange attached); a step that would write row ``per_batch`` makes ``run_device`` / ``step_device`` raise ValueError
        before it is enqueued."""
        if not on:
            self._met_on = False
            if getattr(self, "_pipe", None) is not None:
                check(lib().zt_pipeline_set_metrics(self._pipe, None, None, C.c_int64(0)), "zt_pipeline_set_metrics")
                # the tensors go back to the allocator behind the last kernel that writes them
                check(lib().zt_pipeline_metrics(self._pipe, stream_ptr(), None), "zt_pipeline_metrics")
            self._met_sum = self._met_rows = None
            return
        if getattr(self, "_pipe", None) is None:
            raise RuntimeError("enable_metrics needs enable_pipeline()")
        if not getattr(self, "_score_on", False):
            raise RuntimeError("enable_metrics needs enable_scoring()")
        if int(per_batch) < 0:
            raise ValueError("per_batch must be >= 0")
        check(lib().zt_pipeline_metrics(self._pipe, stream_ptr(), None), "zt_pipeline_metrics")      # (as above, for the old ones)
        self._met_sum = torch.zeros(3, dtype=torch.float64, device=self.device)
        self._met_rows = torch.zeros((int(per_batch), 3), dtype=torch.float64, device=self.device) if per_batch > 0 else None
        self._met_on = True
        try:
            self._pipe_metrics_sync()
        except Exception:
            self._met_on = False
            self._met_sum = self._met_rows = None
            raise

    def _pipe_metrics_sync(self):
        """(Re-)arm the metrics tail on the pipeline at hand: accumulator and table zeroed, the batch counter at 0."""
        if getattr(self, "_pipe", None) is None or not getattr(self, "_met_on", False):
            return
        self._met_sum.zero_()
        if self._met_rows is not None:
            self._met_rows.zero_()
        check(lib().zt_pipeline_set_metrics(self._pipe, ptr(self._met_sum), ptr(self._met_rows),
                                            C.c_int64(0 if self._met_rows is None else self._met_rows.shape[0])),
              "zt_pipeline_set_metrics")
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream != self.main_stream.cuda_stream:      # the steps that follow are ordered behind the zeroing
            self.main_stream.wait_stream(cur)

    def metrics(self, reset=False):
        """(sum, n, per_batch) of the batches measured since ``enable_metrics`` (or the last reset): the float64 [3] sums of
        (AP, AUC, accuracy), the number of batches n (an int the library counts on the host) and the [n, 3] rows of the
        per-batch table or None -- device tensors, valid on the caller's current stream (zt_pipeline_metrics makes it wait for
        the last metrics kernel); no host synchronisation.  Without ``reset`` they are the live buffers, which later steps go
        on writing; ``reset=True`` returns copies, then zeroes the accumulator and the counter on that stream."""
        if getattr(self, "_pipe", None) is None or not getattr(self, "_met_on", False):
            raise RuntimeError("metrics() needs enable_metrics()")
        n = C.c_int64()
        check(lib().zt_pipeline_metrics(self._pipe, stream_ptr(), C.byref(n)), "zt_pipeline_metrics")
        n = int(n.value)
        total, rows = self._met_sum, (self._met_rows[:n] if self._met_rows is not None else None)
        if reset:
            total, rows = total.clone(), (rows.clone() if rows is not None else None)
            self._pipe_metrics_sync()
        return total, n, rows

    def _pipe_scoring_sync(self, force=False):
        if getattr(self, "_pipe", None) is None:
            return
        if not getattr(self, "_score_on", False):
            if force:
                check(lib().zt_pipeline_set_scoring(self._pipe, None, None, None), "zt_pipeline_set_scoring")
            return
        max_b = self._pipe_args[1]
        st = self._affinity_state(max_b, "pipe")
        if st is None:
            raise ValueError("no HIP scorer for hidden width %d" % self.affinity_score.fc1.weight.shape[0])
        st, w, ready = st
        if ready and not force and getattr(self, "_pipe_score_set", False):
            return
        if getattr(self, "_prob_buf", None) is None or self._prob_buf.numel() < 4 * max_b:
            self._prob_buf = torch.zeros(4 * max_b, dtype=torch.float32, device=self.device)
        check(lib().zt_pipeline_set_scoring(self._pipe, C.byref(w), ptr(st["ws"]), ptr(self._prob_buf)), "zt_pipeline_set_scoring")
        self._pipe_score_set = True

    # -- the step as ONE native call (csrc/pipeline.hip): P1 of batch b+1 on a side stream beside P2 + P3 of batch b
    def enable_pipeline(self, on=True, tppr_cus=0, max_batch=16384, group=1):
        """Create (or drop) the native step pipeline.  ``tppr_cus`` > 0 pins the T-PPR stream to the first
        tppr_cus compute units (CU mask) and everything else to the rest; callers run their own work on
        ``self.main_stream``.  With it, ``step_device`` takes ``prefetch`` (the NEXT batch: its T-PPR query is
        issued at once -- it must be the batch of the next call) and ``plan`` (the one after it), or ``ahead`` = the
        list of batches that follow, in order.  ``group`` > 1 (streaming strategy): the T-PPR update of that many
        consecutive batches runs as one launch (zt_pipeline_set_group); 3 * group + 1 batches of ``ahead`` keep it full
        (synth.pipeline_look)."""
        if getattr(self, "_pipe", None) is not None:
            torch.cuda.synchronize(self.device)
            check(lib().zt_pipeline_destroy(self._pipe))
        if getattr(self, "_xchg", None) is not None:
            check(lib().zt_exchange_destroy(self._xchg))
        self._xchg = None
        self._xchg_args = None
        self._pipe = None
        self._pipe_sig = None
        self._pipe_keep = None
        self._pipe_stats = None
        self._batch_cache = collections.OrderedDict()
        self.main_stream = None
        if not on:
            return
        self._pipe_args = (int(tppr_cus), int(max_batch))
        self._pipe_group = int(group)
        self._pipe_refresh(create=True)
        self._pipe_score_set = False
        self._pipe_scoring_sync(force=True)
        self._pipe_metrics_sync()

    # -- multi-GPU: the row exchange INSIDE the native step (csrc/exchange.hip); SURVEY.md 8e
    def enable_exchange(self, rank, world, transport="rccl", with_messages=False, group=None, shm_name=None):
        """Every step of the native pipeline ends with the all-gather of the memory rows the ranks rewrote (and their scatter
        and projected-row refresh), enqueued by the library itself: ``step_device(rows=, positions=)`` and ``run_device`` of
        a sharded run then need no torch.distributed call between steps.  transport "rccl": one rank per GPU, the
        communicator's id is broadcast over ``group`` (torch.distributed); "shm": ranks sharing ONE GPU (tests, rehearsals),
        a POSIX shared-memory segment named ``shm_name``.  ``with_messages``: also exchange the message rows (only needed
        to compare that table across ranks: the eval protocol never reads another rank's messages).  Collective."""
        import torch.distributed as dist
        if getattr(self, "_pipe", None) is None:
            raise RuntimeError("enable_exchange needs enable_pipeline()")
        max_b = self._pipe_args[1]
        m = self.memory
        d = _capi.ExchangeDesc()
        d.rank, d.world, d.with_messages = int(rank), int(world), 1 if with_messages else 0
        d.cap_rows = (2 * max_b + world - 1) // world
        keep = None
        if transport == "rccl":
            uid = torch.zeros(128, dtype=torch.uint8)
            if rank == 0:
                check(lib().zt_exchange_unique_id(ptr(uid), C.c_int64(128)), "zt_exchange_unique_id")
            if world > 1:
                on_gpu = dist.get_backend(group) == "nccl"
                t = uid.to(self.device) if on_gpu else uid
                dist.broadcast(t, 0, group=group)
                uid = t.cpu()
            keep = uid.numpy().tobytes()
            d.transport = _capi.XCHG_RCCL
            d.unique_id = C.cast(C.c_char_p(keep), C.c_void_p)
        elif transport == "shm":
            if not shm_name:
                raise ValueError("transport 'shm' needs shm_name")
            keep = shm_name.encode()
            d.transport = _capi.XCHG_SHM
            d.shm_name = keep
        else:
            raise ValueError("transport must be 'rccl' or 'shm'")
        d.memory, d.last_update, d.messages, d.msg_ts = (m.memory.data_ptr(), m.last_update.data_ptr(), m.messages.data_ptr(),
                                                         m.timestamps.data_ptr())
        d.D, d.msg_dim = self.memory_dimension, m.messages.shape[1]
        h = C.c_void_p()
        if transport == "shm" and world > 1 and dist.is_available() and dist.is_initialized():
            # rank 0 makes the segment (an old one of that name is removed first, the new one starts as zeros); the others
            # open it once it exists: never a segment a killed run left behind (csrc/exchange.hip)
            if rank == 0:
                check(lib().zt_exchange_create(C.byref(h), C.byref(d)), "zt_exchange_create")
            dist.barrier(group=group)
            if rank != 0:
                check(lib().zt_exchange_create(C.byref(h), C.byref(d)), "zt_exchange_create")
        else:
            check(lib().zt_exchange_create(C.byref(h), C.byref(d)), "zt_exchange_create")
        self._xchg = h
        self._xchg_args = (int(rank), int(world), bool(with_messages))
        check(lib().zt_pipeline_set_exchange(self._pipe, h), "zt_pipeline_set_exchange")

    def _pipe_signature(self):
        """Everything the native pipeline holds pointers to: (tables, weight versions)."""
        # identity of every table / handle object and in-place version of every weight (the objects are kept
        # alive by _pipe_keep, so an id cannot be recycled while it is part of the signature)
        em, m, g = self.embedding_module, self.memory, self.memory_updater.memory_updater
        tables = (id(m.memory), m.memory._version, id(m.last_update), id(m.messages), id(m.timestamps), id(m._flag_buf),
                  id(self.edge_raw_features), getattr(em, "_proj_serial", 0),
                  id(em._proj["table"]) if em._proj is not None else 0, id(em._status),
                  id(em._ws), id(self.memory_updater._ws),      # the workspaces the descriptor points into (they are
                                                                # replaced when a call outside the pipeline needs more)
                  id(em.tppr_finder._live) if em.tppr_strategy == "streaming" else id(em.neighbor_finder))
        weights = tuple((id(t), t._version) for t in (em.fc1.weight, em.fc1.bias, em.fc2.weight, em.fc2.bias,
                                                      em.fc1_source.weight, em.fc1_source.bias, em.fc2_source.weight,
                                                      em.fc2_source.bias, g.weight_ih, g.weight_hh, g.bias_ih, g.bias_hh))
        return tables, weights

    def _pipe_refresh(self, create=False):
        """(Re)build the descriptor when a table was replaced (restore_memory, __init_memory__, a new neighbour
        finder, restore_tppr) or a weight changed in place; cheap when nothing did.  Runs on the main stream."""
        sig = self._pipe_signature()
        if not create and sig == self._pipe_sig:
            return
        em, m, mu = self.embedding_module, self.memory, self.memory_updater
        tppr_cus, max_b = self._pipe_args
        D, F, T = self.memory_dimension, self.n_edge_features, self.time_dimension
        em._ws_shape = max(3 * max_b, em._ws_shape or 0)
        ws, _, _ = em._workspace(em._ws_shape)
        gws = mu._workspace(2 * max_b, D)
        table = em._projection(m)                       # rebuilt here if the memory or W_m changed
        if em._status is None:
            em._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        d = _capi.PipelineDesc()
        if em.tppr_strategy == "streaming":
            d.tppr = em.tppr_finder._live.h
        else:
            em.ensure_pruning_workspace()               # the side stream's query takes the workspace form through this handle
            d.csr = em.neighbor_finder._h
            d.width, d.depth = em.width, em.depth
            for q, (a, bb) in enumerate(zip(em.alpha_list, em.beta_list)):
                d.alpha[q], d.beta[q] = float(a), float(bb)
        d.memory, d.last_update, d.messages, d.msg_ts = (m.memory.data_ptr(), m.last_update.data_ptr(),
                                                         m.messages.data_ptr(), m.timestamps.data_ptr())
        d.flags, d.scratch, d.efeat = m._flag_buf.data_ptr(), self._scratch.data_ptr(), self.edge_raw_features.data_ptr()
        d.num_nodes, d.num_edges = m.n_nodes, self.edge_raw_features.shape[0]
        d.D, d.F, d.T, d.M, d.k = D, F, T, em.n_tppr, em.k
        d.ew, d.gw = em._embed_weights(), mu._weights()
        d.embed_ws, d.gru_ws = ws.data_ptr(), gws.data_ptr()
        d.proj_table = table.data_ptr() if table is not None else None
        d.status = em._status.data_ptr()
        d.max_B = max_b
        self._pipe_keep = (ws, gws, table, d, m.memory, m.last_update, m.messages, m.timestamps, m._flag_buf,
                           em.tppr_finder._live if em.tppr_strategy == "streaming" else em.neighbor_finder)
        if create:
            h = C.c_void_p()
            check(lib().zt_pipeline_create(C.byref(h), C.byref(d), C.c_int32(tppr_cus)), "zt_pipeline_create")
            self._pipe = h
            if getattr(self, "_pipe_group", 1) > 1:
                check(lib().zt_pipeline_set_group(h, C.c_int32(self._pipe_group)), "zt_pipeline_set_group")
            self.main_stream = torch.cuda.ExternalStream(lib().zt_pipeline_main_stream(h), device=self.device)
            self._pipe_cell = _capi.CELL_GRU
        else:
            check(lib().zt_pipeline_update(self._pipe, C.byref(d), C.c_int32(1)), "zt_pipeline_update")
            if getattr(self, "_xchg", None) is not None:      # the exchange follows the tables
                check(lib().zt_exchange_set_tables(self._xchg, ptr(m.memory), ptr(m.last_update), ptr(m.messages),
                                                   ptr(m.timestamps)), "zt_exchange_set_tables")
        cell = getattr(mu, "cell", _capi.CELL_GRU)
        if cell != self._pipe_cell:                     # the memory updater's cell (RNNMemoryUpdater: zt_rnn_update's kernels)
            check(lib().zt_pipeline_set_cell(self._pipe, C.c_int32(cell)), "zt_pipeline_set_cell")
            self._pipe_cell = cell
        em._ws_key = None                               # the pipeline remakes the padded weights at its next step
        mu._ws_key = None
        self._pipe_sig = self._pipe_signature()

    def _batch_struct(self, batch):
        """zt_batch of five device tensors; remembered by the identity of the edge-id tensor (a batch is
        presented three times: as plan, as prefetch, as the current one)."""
        cache = self._batch_cache
        key = id(batch[4])
        hit = cache.get(key)
        if hit is not None and hit[0][4] is batch[4]:
            return hit[1]
        b = _capi.Batch()
        b.src, b.dst, b.neg, b.ts, b.eidx = [t.data_ptr() for t in batch]
        b.B = batch[0].numel()
        # ALL five tensors stay referenced while a slot may still read them on the plan / T-PPR streams (a batch is
        # staged at most 3 * MAX_GROUP steps before its own step; the oldest entries go first)
        while len(cache) >= 64:
            cache.popitem(last=False)
        cache[key] = (tuple(batch), b)
        return b

    def _pipe_step(self, batch, prefetch, plan, rows=None, positions=None, ahead=None):
        """zt_pipeline_step_ahead; returns the embeddings of ``rows`` (valid on the caller's current stream)."""
        if ahead is None:
            ahead = [b for b in (prefetch, plan if prefetch is not None else None) if b is not None]
        caller = torch.cuda.current_stream(self.device)
        if caller.cuda_stream == self.main_stream.cuda_stream:
            return self._pipe_step_main(batch, ahead, rows, positions)
        self.main_stream.wait_stream(caller)            # inputs produced on the caller's stream
        with torch.cuda.stream(self.main_stream):
            out = self._pipe_step_main(batch, ahead, rows, positions)
        caller.wait_stream(self.main_stream)
        out.record_stream(caller)
        return out

    def _ahead_array(self, ahead):
        """ctypes array of zt_batch for the batches that follow; remembered by the identity of its members."""
        key = tuple(id(b[4]) for b in ahead)
        hit = self._batch_cache.get(key)
        if hit is not None and all(x[4] is b[4] for x, b in zip(hit[0], ahead)):
            return hit[1]
        arr = (_capi.Batch * max(1, len(ahead)))()
        for q, b in enumerate(ahead):
            arr[q] = self._batch_struct(b)
        while len(self._batch_cache) >= 64:
            self._batch_cache.popitem(last=False)
        self._batch_cache[key] = ([tuple(b) for b in ahead], arr)
        return arr

    def _pipe_want_stats(self, on):
        """average_topk from the slot's weights (zt_pipeline_set_stats), only while somebody asks for it"""
        if bool(on) == (self._pipe_stats is not None):
            return
        em = self.embedding_module
        if on:
            self._pipe_stats = torch.zeros(1, dtype=torch.float32, device=self.device)
            check(lib().zt_pipeline_set_stats(self._pipe, ptr(self._pipe_stats)), "zt_pipeline_set_stats")
            em._avg_topk_t = self._pipe_stats
        else:
            check(lib().zt_pipeline_set_stats(self._pipe, None), "zt_pipeline_set_stats")
            self._pipe_stats = None

    def pipeline_outstanding(self):
        """Batches whose T-PPR update ran ahead of their step (0 without a pipeline)."""
        if getattr(self, "_pipe", None) is None:
            return 0
        return int(lib().zt_pipeline_outstanding(self._pipe))

    def pipeline_tail_gates(self):
        """Steps whose GRU kernel carried the next batch's T-PPR gate at its tail (zt_pipeline_tail_gates; 0 without a pipeline)."""
        if getattr(self, "_pipe", None) is None:
            return 0
        return int(lib().zt_pipeline_tail_gates(self._pipe))

    def _pipe_step_main(self, batch, ahead, rows, positions):
        self._pipe_refresh()
        if getattr(self, "_score_on", False):
            self._pipe_scoring_sync()
        B = batch[0].numel()
        r0, r1 = rows if rows is not None else (0, 3 * B)
        p0, p1 = positions if positions is not None else (0, 2 * B)
        em = self.embedding_module
        out = torch.empty((r1 - r0, self.embedding_dimension * (em.n_tppr + 1)), dtype=torch.float32, device=self.device)
        cur = self._batch_struct(batch)
        arr = self._ahead_array(ahead)
        check(lib().zt_pipeline_step_ahead(self._pipe, C.byref(cur), arr, C.c_int32(len(ahead)), C.c_int64(r0),
                                           C.c_int64(r1), C.c_int64(p0), C.c_int64(p1), ptr(out)), "zt_pipeline_step")
        return out

    def prepare_run(self, batches):
        """The ctypes view of a list of batches (five device tensors each) for ``run_device``: made once, outside a timed
        region.  The tensors must stay alive while a run may still read them."""
        arr = (_capi.Batch * max(1, len(batches)))()
        for q, b in enumerate(batches):
            arr[q].src, arr[q].dst, arr[q].neg, arr[q].ts, arr[q].eidx = [x.data_ptr() for x in b]
            arr[q].B = b[0].numel()
        return arr, len(batches), [tuple(b) for b in batches]

    @torch.no_grad()
    def run_device(self, prepared, out=None, look=None):
        """n consecutive eval-mode steps over whole batches as ONE native call (zt_pipeline_run): the batch loop of
        evaluation/evaluation.py:19-45 without a Python iteration per batch.  ``prepared`` = ``prepare_run(batches)``.
        out: None (one [3 B, H] buffer overwritten by every step -- for callers after the scores or the final state), or a
        [n, 3 B, H] float32 tensor that receives every step's embeddings.  Call from ``self.main_stream``; the streaming
        T-PPR state ends exactly behind the last batch given."""
        if getattr(self, "_pipe", None) is None:
            raise RuntimeError("run_device needs enable_pipeline()")
        if not self.test_mode:
            self.update_memory_in_test(self.memory)
            self.test_mode = True
        arr, n, keep = prepared
        if n == 0:
            return out
        self._pipe_refresh()
        if getattr(self, "_score_on", False):
            self._pipe_scoring_sync()
        self._pipe_want_stats(False)
        H = self.embedding_dimension * (self.embedding_module.n_tppr + 1)
        Bmax = max(int(arr[q].B) for q in range(n))
        rows_max = 3 * Bmax
        if getattr(self, "_xchg_args", None) is not None:          # a sharded run: step b writes this rank's rows only
            rk, wd, _ = self._xchg_args
            rows_max = max((3 * int(arr[q].B) * (rk + 1)) // wd - (3 * int(arr[q].B) * rk) // wd for q in range(n))
        if out is None:
            buf = getattr(self, "_run_scratch", None)
            if buf is None or buf.numel() < max(1, rows_max) * H:
                buf = self._run_scratch = torch.empty(max(1, rows_max) * H, dtype=torch.float32, device=self.device)
            stride = 0
        else:
            if out.shape != (n, rows_max, H) or out.dtype != torch.float32 or not out.is_contiguous():
                raise ValueError("out must be a contiguous float32 [n, rows, H] tensor (rows = 3 B, or this rank's shard of them)")
            buf, stride = out, rows_max * H
        self._run_keep = keep
        check(lib().zt_pipeline_run(self._pipe, arr, C.c_int32(n), C.c_int32(3 * self._pipe_group + 1 if look is None else look),
                                    ptr(buf), C.c_int64(stride)), "zt_pipeline_run")
        return out

    @torch.no_grad()
    def step_device(self, src_d, dst_d, neg_d, ts_d, eidx_d, check_status=False, prefetch=None, plan=None,
                    stats=False, rows=None, positions=None, ahead=None):
        """One eval-mode batch (tgn_model.py:124-174 with train=False), inputs
        int32/int32/int32/float64/int64 CUDA tensors, no host sync unless
        ``check_status``.  Returns the [3B, D*(n_tppr+1)] embeddings (or those of ``rows`` = (lo, hi);
        ``positions`` = (lo, hi) restricts the memory update to winners at those batch positions: the two
        are how a multi-GPU run shards a batch).  With ``enable_pipeline``: ``prefetch`` = the next batch's
        five tensors (queried at once), ``plan`` = the one after it -- or ``ahead`` = the list of the batches that
        follow (see ``enable_pipeline(group=)``); call from ``self.main_stream``."""
        if not self.test_mode:
            self.update_memory_in_test(self.memory)
            self.test_mode = True
        em = self.embedding_module
        B = src_d.numel()
        if getattr(self, "_pipe", None) is not None:
            self._pipe_want_stats(stats and rows is None)
            emb = self._pipe_step((src_d, dst_d, neg_d, ts_d, eidx_d), prefetch, plan, rows, positions, ahead)
        else:
            nodes_d = torch.cat([src_d, dst_d, neg_d])
            ts3 = ts_d if em.tppr_strategy == "streaming" else torch.cat([ts_d, ts_d, ts_d])
            r0, r1 = rows if rows is not None else (0, 3 * B)
            if em.tppr_strategy == "pruning" and rows is not None:       # rows are independent: query the shard only
                on, oe, od, ow = em.pruning_topk_device(nodes_d[r0:r1].contiguous(), ts3[r0:r1].contiguous(),
                                                        check_status=check_status)
            else:
                on, oe, od, ow = em.topk_device(nodes_d, ts3, eidx_d, check_status=check_status)
                if stats:                                # average_topk (modules/embedding_module.py:232-233)
                    em._avg_topk_t = ow[0, : 2 * B].sum(dim=1).mean()
                if rows is not None:
                    on, oe, od, ow = [t[:, r0:r1].contiguous() for t in (on, oe, od, ow)]
            emb = em.embed_device(self.memory.memory, nodes_d[r0:r1].contiguous() if rows is not None else nodes_d,
                                  on, oe, od, ow, check_status=check_status, memory_obj=self.memory)
            self.store_messages_device(src_d, dst_d, ts_d, eidx_d, pos_range=positions)
            self.memory_updater.update_device(self.memory, nodes_d[: 2 * B], 2 * B)      # [src | dst], flagged once each
        if check_status:
            self.check_status()
        return emb

    def check_status(self):
        """The T-PPR handle's latch and the step kernels' status words, read on the host (a synchronisation): IndexError for an
        id out of range, ZebraError for a bounded in-kernel wait that gave up; the words are cleared.  ``step_device(check_status=
        True)`` ends with it; after ``run_device`` call it once."""
        em = self.embedding_module
        if em.tppr_strategy == "streaming":
            em.tppr_finder.check_status()
        st = int(self._status.item()) or (int(em._status.item()) if em._status is not None else 0)
        if st != 0:
            self._status.zero_()
            if em._status is not None:
                em._status.zero_()
            if st == _capi.ZT_ERR_TIMEOUT:
                raise _capi.ZebraError("a kernel of the step gave up a bounded in-kernel wait (status %d): the step's memory "
                                       "update is incomplete" % st)
            raise IndexError("node / edge id out of range (status %d)" % st)

    # ------------------------------------------------------------------ reference surface
    def compute_temporal_embeddings(self, source_nodes, destination_nodes, negative_nodes, edge_times, edge_idxs,
                                    n_neighbors, train, edge_sel=None):
        self.batch_counter += 1
        n_samples = len(source_nodes)
        positives = np.concatenate([source_nodes, destination_nodes])
        unique_positives = np.unique(positives)
        self.n_update_memory += len(positives)
        d = self.device
        # the batch goes to the device in ONE asynchronous transfer (a training step used to make eight synchronous ones)
        host = [np.ascontiguousarray(source_nodes, np.int32), np.ascontiguousarray(destination_nodes, np.int32),
                np.ascontiguousarray(edge_times, np.float64), np.ascontiguousarray(edge_idxs, np.int64),
                np.ascontiguousarray(unique_positives, np.int32)]
        if negative_nodes is not None:
            host.append(np.ascontiguousarray(negative_nodes, np.int32))
        dev = _capi.to_device(d, host)
        src_d, dst_d, ts_d, eidx_d, upos_d = dev[:5]

        if not train:
            if negative_nodes is None:
                raise ValueError("the accelerated eval path expects negatives (tgn_model.py:132)")
            neg_d = dev[5]
            node_embedding = self.step_device(src_d, dst_d, neg_d, ts_d, eidx_d, check_status=True, stats=True)
        else:
            if self.pipeline_outstanding():
                raise RuntimeError("the step pipeline has queried %d batches ahead: their T-PPR updates are applied "
                                   "already; step them (or rebuild the pipeline) before a training batch"
                                   % self.pipeline_outstanding())
            self.test_mode = False
            nodes = np.concatenate([source_nodes, destination_nodes, negative_nodes])
            timestamps = np.concatenate([edge_times, edge_times, edge_times])
            # edge_sel (data-parallel training): embed the rows of these edges only; state updates cover the batch
            row_sel = None
            if edge_sel is not None:
                es = torch.as_tensor(np.asarray(edge_sel), device=d).long()
                row_sel = torch.cat([es, es + n_samples, es + 2 * n_samples])
                n_samples = int(es.numel())
            on_device = None
            if negative_nodes is not None:
                on_device = (torch.cat([src_d, dst_d, dev[5]]), ts_d.repeat(3), eidx_d)
            node_embedding = self.embedding_module.compute_embedding_tppr_ensemble(
                memory=self.memory, source_nodes=nodes, timestamps=timestamps, edge_idxs=edge_idxs,
                memory_updater=self.memory_updater, train=True, row_sel=row_sel, on_device=on_device)
            # update memory without gradients, THEN collect raw messages (:155-168)
            with torch.no_grad():
                self.memory_updater.update_device(self.memory, upos_d, upos_d.numel())
            with torch.no_grad():
                self.store_messages_device(src_d, dst_d, ts_d, eidx_d)
        self._last_node_embedding = node_embedding if edge_sel is None else None
        self._last_node_block = node_embedding                           # [3 n_samples, H]: what the three slices are views of
        return (node_embedding[:n_samples], node_embedding[n_samples:2 * n_samples], node_embedding[2 * n_samples:])

    def compute_edge_probabilities(self, source_nodes, destination_nodes, negative_nodes, edge_times, edge_idxs,
                                   n_neighbors, train):
        n_samples = len(source_nodes)
        s, dd, n = self.compute_temporal_embeddings(source_nodes, destination_nodes, negative_nodes, edge_times,
                                                    edge_idxs, n_neighbors, train)
        if not train and not torch.is_grad_enabled() and s.is_cuda:
            # eval: the HIP scorer (csrc/scoring.hip) on the [3B, H] block the step returned; same shapes as below
            if getattr(self, "_pipe", None) is not None and getattr(self, "_score_on", False):
                prob = self.last_prob()                                  # the native step has scored this batch already
                return prob[:n_samples].unsqueeze(1), prob[n_samples:].unsqueeze(1)
            full = getattr(self, "_last_node_embedding", None)           # the [3B, H] block s / dd / n are slices of
            if full is None or full.data_ptr() != s.data_ptr() or full.shape[0] != 3 * n_samples:
                full = torch.cat([s, dd, n])
            prob = self.score_device(full)
            return prob[:n_samples].unsqueeze(1), prob[n_samples:].unsqueeze(1)
        if train and link_score_plan(s.device.type, s.dtype, s.shape[1], getattr(self, "fused_scoring", True)) == "hip":
            full = getattr(self, "_last_node_block", None)               # the [3B, H] block s / dd / n are slices of
            if full is None or full.data_ptr() != s.data_ptr() or full.shape[0] != 3 * n_samples or not full.is_contiguous():
                full = torch.cat([s, dd, n])
            return self.score_train(full)
        return self._score_pairs(s, dd, n)

    def compute_edge_loss(self, source_nodes, destination_nodes, negative_nodes, edge_times, edge_idxs, n_neighbors):
        """(loss, pos_prob, neg_prob) of a training batch: train.py:212-213 in one call -- compute_edge_probabilities(train=True)
        and BCELoss of the positive pairs against ones plus BCELoss of the negative pairs against zeros.  Where link_score_plan
        says "hip" the [2B] vector of _HipLinkScore goes straight into _HipLinkBCE (csrc/train_tail.hip): no slice, squeeze or
        cat node enters the graph; otherwise the probabilities' composition with losses.link_bce_loss.  pos_prob and neg_prob
        are detached [B, 1] views for the caller's metrics.  The single negative's T-PPR row is emitted by the stream in batch
        order (role 3 of its edge); compute_rank_loss, with many negatives, reads theirs from the state before the batch."""
        n_samples = len(source_nodes)
        s, dd, n = self.compute_temporal_embeddings(source_nodes, destination_nodes, negative_nodes, edge_times, edge_idxs,
                                                    n_neighbors, True)
        if n_samples and link_score_plan(s.device.type, s.dtype, s.shape[1], getattr(self, "fused_scoring", True)) == "hip":
            full = getattr(self, "_last_node_block", None)               # (as compute_edge_probabilities)
            if full is None or full.data_ptr() != s.data_ptr() or full.shape[0] != 3 * n_samples or not full.is_contiguous():
                full = torch.cat([s, dd, n])
            a = self.affinity_score
            prob = _HipLinkScore.apply(full, a.fc1.weight, a.fc1.bias, a.fc2.weight, a.fc2.bias)
            loss = _HipLinkBCE.apply(prob)
            prob = prob.detach()
            return loss, prob[:n_samples].unsqueeze(1), prob[n_samples:].unsqueeze(1)
        pos, neg = self._score_pairs(s, dd, n)
        return link_bce_loss(pos, neg), pos.detach(), neg.detach()

    def compute_rank_loss(self, source_nodes, destination_nodes, negative_nodes, edge_times, edge_idxs, n_neighbors,
                          mode="softmax", edge_sel=None):
        """(loss, logits) of ONE training step that ranks every edge's destination against K negatives: ``negative_nodes`` is
        [B, K], K >= 1, -1 = absent (a filtered sampler drops a source's true partners this way) -- a numpy array, or an int32
        tensor such as zebra_amd.sampling.NegativeSampler.sample_for returns, which is read back once; ``mode`` is listwise_loss's
        ("softmax": cross-entropy of column 0 over the present columns; "bce": compute_edge_loss's loss with the negatives'
        term averaged over all present negatives).  logits [B, 1 + K] (column 0: the destination; -inf: absent) is detached,
        for the caller's metrics.
        The negatives' convention is eval_edge_ranking's, NOT compute_edge_loss's: the T-PPR rows of the present negatives are
        read (``query_device``), each at its edge's timestamp, from the state BEFORE the batch, where compute_edge_loss's
        single negative is emitted by the stream in batch order -- a negative that is an endpoint of an earlier edge of
        the batch sees that edge there and not here.  A negative that is no endpoint of the batch reads the same row either
        way.  Then the step is compute_temporal_embeddings(train=True)'s: the T-PPR stream runs over [src | dst] (negatives
        never write state), GraphDiffusionEmbedding._train_forward embeds the 2B + n_present rows at once, the memory update
        and the message store follow, score_many_train scores the sources against [destinations | negatives] and
        listwise_loss finishes.  ValueError for negatives that are not [B, K >= 1] or for ``edge_sel`` (data-parallel shares
        are not covered); RuntimeError with the native pipeline (and so an exchange) enabled."""
        if edge_sel is not None:
            raise ValueError("compute_rank_loss does not cover data-parallel shares (edge_sel)")
        if torch.is_tensor(negative_nodes):                              # NegativeSampler.sample_for's rows: read back once --
            negative_nodes = negative_nodes.detach().cpu().numpy()       # the index below is built on the host
        neg = np.asarray(negative_nodes)
        B = len(source_nodes)
        if neg.ndim != 2 or neg.shape[0] != B or neg.shape[1] < 1:
            raise ValueError("compute_rank_loss takes negative_nodes [B, K] with K >= 1 (-1: absent)")
        if getattr(self, "_pipe", None) is not None or getattr(self, "_xchg", None) is not None:
            raise RuntimeError("compute_rank_loss does not cover the native pipeline or its exchange: call "
                               "enable_pipeline(False) first")
        K = neg.shape[1]
        self.batch_counter += 1
        positives = np.concatenate([source_nodes, destination_nodes])
        self.n_update_memory += len(positives)
        self.test_mode = False
        # the index of the scorer and the negatives' (node, time) list, on the host: nothing of it waits for the device
        present = neg >= 0
        n_present = int(present.sum())
        cand_idx = np.full((B, 1 + K), -1, np.int32)
        cand_idx[:, 0] = np.arange(B, dtype=np.int32)                    # emb_c = [destinations | present negatives]
        cand_idx[:, 1:][present] = B + np.arange(n_present, dtype=np.int32)
        neg_ts = np.broadcast_to(np.asarray(edge_times, np.float64).reshape(B, 1), (B, K))[present]
        src_d, dst_d, ts_d, eidx_d, upos_d, negn_d, negts_d, cand_d = _capi.to_device(self.device, [
            np.ascontiguousarray(source_nodes, np.int32), np.ascontiguousarray(destination_nodes, np.int32),
            np.ascontiguousarray(edge_times, np.float64), np.ascontiguousarray(edge_idxs, np.int64),
            np.ascontiguousarray(np.unique(positives), np.int32), np.ascontiguousarray(neg[present], np.int32),
            np.ascontiguousarray(neg_ts, np.float64), cand_idx])
        emb = self.embedding_module.compute_embedding_tppr_ensemble(
            memory=self.memory, source_nodes=positives, timestamps=None, edge_idxs=edge_idxs, memory_updater=self.memory_updater,
            train=True, on_device=(torch.cat([src_d, dst_d]), ts_d.repeat(2), eidx_d), extra=(negn_d, negts_d))
        # update memory without gradients, THEN collect raw messages (:155-168), as compute_temporal_embeddings(train=True)
        with torch.no_grad():
            self.memory_updater.update_device(self.memory, upos_d, upos_d.numel())
            self.store_messages_device(src_d, dst_d, ts_d, eidx_d)
        self._last_node_embedding = self._last_node_block = None
        logits = self.score_many_train(emb[:B], emb[B:], cand_d)
        return listwise_loss(logits, None, mode), logits.detach()

    def update_memory(self, memory, positives):
        with torch.no_grad():
            self.memory_updater.update_memory(memory, positives)

    def update_memory_in_test(self, memory):
        with torch.no_grad():
            self.memory_updater.update_memory_in_test(memory)

    def get_updated_memory(self, memory):
        return self.memory_updater.get_updated_memory(memory)

    def set_neighbor_finder(self, neighbor_finder):
        self.neighbor_finder = neighbor_finder
        self.embedding_module.neighbor_finder = neighbor_finder
