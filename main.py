"""Stage-2 driver with the reference's CLI, Trainer surface and log lines (reference main.py),
running on the gfx950 HIP kernels of llmrec_amd.

    python main.py --dataset netflix_valid_item --data_path ./data/ [reference flags ...]

What differs from the reference, by design (results are unchanged):
  * the graph is turned into device CSR once; the hot loop never touches COO tensors;
  * each of the 8 BPR + prune losses per step is ONE kernel with on-device selection - the
    reference copies the scores to the host and argsorts them there (main.py:159), 8 syncs/step;
  * losses are accumulated on the device and read once per epoch (the reference calls float()
    on four tensors every step, main.py:280-283);
  * augmented_sample_dict is unpickled once, not every step (main.py:216);
  * the two pickles the reference re-writes into the dataset directory at start-up
    (main.py:66,78) are not written.
Modes:
  * default: the reference's own sample stream (utility/load_data.py: same seed -> the same (users, pos, neg) triples as the
    reference, drawn on the host), one H2D copy of the batch, the fused step replayed from a captured HIP graph, the evaluation
    from another; LLMREC_GRAPH=0 issues the same launches one by one, LLMREC_FUSED=0 runs the per-op autograd path;
  * LLMREC_DEVICE_SAMPLER=1: the HIP sampler inside the step graph (distribution-equivalent, not stream-equivalent to the
    reference's host RNG): an epoch is n_batch / 4 graph launches and nothing else - the mode bench.py's headline times.
"""
from datetime import datetime
import math
import os

import pickle
import random
import sys
from time import time

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn
import torch.nn.functional as F

from utility.parser import parse_args
from Models import MM_Model, Decoder
from utility.batch_test import *          # data_generator, test_torch, Ks, ... (reference main.py:28)
from utility.logging import Logger
from llmrec_amd import engine, ops

args = parse_args()
if torch.cuda.is_available():                              # --gpu_id (reference parser.py:22) selects the device
    if not 0 <= args.gpu_id < torch.cuda.device_count():   # a mistyped id must not land (and contend) on GPU 0 silently
        raise SystemExit("--gpu_id %d: this process sees %d GPU(s)" % (args.gpu_id, torch.cuda.device_count()))
    torch.cuda.set_device(args.gpu_id)
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")



def USE_GRAPH():
    """LLMREC_GRAPH (default 1): the fused step and the evaluation are replayed from captured HIP graphs; 0 = the same launches
    issued one by one from Python (debugging, and the A/B of the graph itself)."""
    return os.environ.get("LLMREC_GRAPH", "1") == "1"


ATTRIBUTE_KEYS = {                                         # reference main.py:69-72
    'preprocessed_raw_MovieLens': ['title', 'genre', 'director', 'country', 'language'],
    'netflix_valid_item': ['year', 'title', 'director', 'country', 'language'],
}


def _progress(it):
    try:
        from tqdm import tqdm
        return tqdm(it)
    except Exception:
        return it


def test_full_on_device(ua_embeddings, ia_embeddings, users_to_test, is_val, topk=None):
    """--test_flag full (reference utility/batch_test.py:38-68,104-108) without test_torch's host loop over score blocks: the ranking
    metrics exactly as the 'part' evaluation computes them (masked top-K, hits and per-user metrics on the device), and the full-rank AUC of
    every user by llmrec_score_auc_f32 - integer pair counts on the device, summed by a fixed tree into one pinned double. No score block
    leaves the device and sklearn is not needed. topk: optional (query tensor, ranked lists) already computed for exactly users_to_test."""
    from llmrec_amd import ops
    result = {'precision': np.zeros(len(Ks)), 'recall': np.zeros(len(Ks)), 'ndcg': np.zeros(len(Ks)),
              'hit_ratio': np.zeros(len(Ks)), 'auc': 0.}
    n = len(users_to_test)
    if n == 0:
        return result
    st = data_generator.device_state(ua_embeddings.device)
    q, idx = topk if topk is not None else topk_lists(ua_embeddings, ia_embeddings, list(users_to_test))
    rp, ci = st["val"] if is_val else st["test"]
    sums = ops.topk_metrics(idx, ops.topk_hits(idx, q, rp, ci), q, rp, Ks).sum(0).cpu().numpy() / n
    for j, k in enumerate(('precision', 'recall', 'ndcg', 'hit_ratio')):
        result[k] = sums[j]
    auc_sum = torch.zeros(1, dtype=torch.float64).pin_memory()
    ops.score_auc(ua_embeddings, ia_embeddings, q, st["train"], (rp, ci), out=auc_sum)
    torch.cuda.current_stream().synchronize()
    result['auc'] = float(auc_sum[0]) / n
    return result


class Trainer(object):
    def __init__(self, data_config):
        self.task_name = "%s_%s_%s" % (datetime.now().strftime('%Y-%m-%d %H:%M:%S'), args.dataset, args.cf_model,)
        self.logger = Logger(filename=self.task_name, is_debug=args.debug)
        self.logger.logging("PID: %d" % os.getpid())
        self.logger.logging(str(args))

        self.mess_dropout = eval(args.mess_dropout)
        self.lr = args.lr
        self.emb_dim = args.embed_size
        self.batch_size = args.batch_size
        self.weight_size = eval(args.weight_size)
        self.n_layers = len(self.weight_size)
        self.regs = eval(args.regs)
        self.decay = self.regs[0]

        root = args.data_path + args.dataset
        self.image_feats = np.load(root + '/image_feat.npy')
        self.text_feats = np.load(root + '/text_feat.npy')
        self.image_feat_dim = self.image_feats.shape[-1]
        self.text_feat_dim = self.text_feats.shape[-1]
        with open(root + '/train_mat', 'rb') as f:
            self.ui_graph = self.ui_graph_raw = pickle.load(f)
        with open(root + '/augmented_user_init_embedding', 'rb') as f:
            user_emb = pickle.load(f)
        self.user_init_embedding = np.array([user_emb[i] for i in range(len(user_emb))])
        if args.dataset not in ATTRIBUTE_KEYS:             # the reference dies with a NameError here
            raise ValueError("--dataset must be one of %s" % sorted(ATTRIBUTE_KEYS))
        with open(root + '/augmented_atttribute_embedding_dict', 'rb') as f:
            attr = pickle.load(f)
        self.item_attribute_embedding = {key: [] for key in ATTRIBUTE_KEYS[args.dataset]}
        for key in attr.keys():
            self.item_attribute_embedding[key] = np.array([attr[key][i] for i in range(len(attr[key]))])
        with open(root + '/augmented_sample_dict', 'rb') as f:
            self.augmented_sample_dict = pickle.load(f)

        self.n_users, self.n_items = self.ui_graph.shape
        self.iu_graph = self.ui_graph.T
        self.ui_graph = self.matrix_to_tensor(self.csr_norm(self.ui_graph, mean_flag=True))
        self.iu_graph = self.matrix_to_tensor(self.csr_norm(self.iu_graph, mean_flag=True))
        self.image_ui_graph = self.text_ui_graph = self.ui_graph
        self.image_iu_graph = self.text_iu_graph = self.iu_graph

        self.model_mm = MM_Model(self.n_users, self.n_items, self.emb_dim, self.weight_size, self.mess_dropout,
                                 self.image_feats, self.text_feats, self.user_init_embedding, self.item_attribute_embedding)
        self.model_mm = self.model_mm.to(device)
        self.decoder = Decoder(self.user_init_embedding.shape[1]).to(device)

        # torch.optim.AdamW(lr) defaults (betas .9/.999, eps 1e-8, weight_decay 0.01), fused HIP kernel
        self.optimizer = ops.FusedAdamW(self.model_mm.parameters(), lr=self.lr)
        self.de_optimizer = torch.optim.AdamW([{'params': self.decoder.parameters()}], lr=args.de_lr)   # never stepped
        self.hyper = engine.Hyper.from_args(args)
        self._on_bpr = None                                   # test hook: called with (mf, emb) of each BPR call
        self._on_epoch = None                                 # test hook: called with (epoch, loss, mf_loss, emb_loss, ret, (t2 - t1, t3 - t2)) per epoch
        self._fused = None
        self._device_sampler = os.environ.get("LLMREC_DEVICE_SAMPLER", "0") == "1"
        self._global_step = 0

    # -- graph helpers (same arithmetic as the reference, host side, once) -----------------------
    def csr_norm(self, csr_mat, mean_flag=False):
        def inv_sqrt(total):
            s = np.power(np.array(total) + 1e-8, -0.5).flatten()
            s[np.isinf(s)] = 0.
            return sp.diags(s)
        left = inv_sqrt(csr_mat.sum(1))
        if mean_flag:
            return left * csr_mat
        return left * csr_mat * inv_sqrt(csr_mat.sum(0))

    def matrix_to_tensor(self, cur_matrix):
        coo = cur_matrix if isinstance(cur_matrix, sp.coo_matrix) else cur_matrix.tocoo()
        indices = torch.from_numpy(np.vstack((coo.row, coo.col)).astype(np.int64))
        values = torch.from_numpy(coo.data)
        return torch.sparse_coo_tensor(indices, values, torch.Size(coo.shape)).to(torch.float32).to(device)

    # -- losses -----------------------------------------------------------------------------------
    def feat_reg_loss_calculation(self, g_item_image, g_item_text, g_user_image, g_user_text):
        coef = args.feat_reg_decay * 0.5 / self.n_items
        return ops.sumsq(coef, [g_item_image, g_item_text, g_user_image, g_user_text])[0]

    def prune_loss(self, pred, drop_rate):
        """Mean of the int((1-drop)*B) smallest entries. The training loop does not call this:
        selection is fused into the BPR kernel (ops.bpr_prune). Kept for the reference surface."""
        keep = int((1 - drop_rate) * len(pred))
        order = torch.argsort(pred.detach(), stable=True)
        return pred[order[:keep]].mean()

    def _bpr(self, user_table, item_table, users, pos_items, neg_items):
        mf, emb = engine.bpr(self.hyper, user_table, item_table, users, pos_items, neg_items)
        return mf, emb, 0.0

    def bpr_loss(self, users, pos_items, neg_items):
        """Reference signature: three gathered [B, d] blocks -> (mf_loss, emb_loss, reg_loss)."""
        B = users.shape[0]
        idx = torch.arange(B, dtype=torch.int64, device=users.device)
        return self._bpr(users, torch.cat([pos_items, neg_items], dim=0), idx, idx, idx + B)

    def sce_criterion(self, x, y, alpha=1):
        x, y = F.normalize(x, p=2, dim=-1), F.normalize(y, p=2, dim=-1)
        return (1 - (x * y).sum(dim=-1)).pow_(alpha).mean()

    def mse_criterion(self, x, y, alpha=3):
        return F.mse_loss(F.normalize(x, p=2, dim=-1), F.normalize(y, p=2, dim=-1))

    # -- evaluation -------------------------------------------------------------------------------
    def test(self, users_to_test, is_val):
        if self.model_mm.training:
            self.model_mm.eval()
        fused = self._fused_step()
        with torch.no_grad():
            if fused:
                # forward + scoring + masked top-K as ONE graph replay per evaluation (LLMREC_EVAL_GRAPH=0: the same launches issued eagerly).
                # Round 6, full Netflix-shaped dataset, tools/eval_probe.py, ms per evaluation [20 back to back | one at a time, host
                # synchronised behind each, as this method runs]: one-stream graph 0.601 | 0.620; eager 0.558 | 0.664 - issued onto an idle
                # GPU the ~40 launches leave the host ~70 us behind the device (graphs on four streams: FusedStep.eval_topk).
                # the query tensor is cached on the CONTENT of the user list (a different list of the same length
                # must not reuse it); the evaluation graph is keyed on that tensor
                own = getattr(self, "_eval_own", None)          # the list train() itself built once and hands in every epoch: trusted by identity
                if own is not None and own[0] is users_to_test and own[1] == len(users_to_test):
                    q = own[2]                                  # (converting 13 k python ints per evaluation cost 0.4 ms of a 1.1 ms evaluation)
                else:
                    users_np = np.asarray(users_to_test, dtype=np.int64)
                    users_key = users_np.tobytes()              # (the list's content as one bytes object: hashed and compared in ~30 us for 13 k users)
                    cache = getattr(self, "_eval_queries", None)
                    if cache is None:
                        cache = self._eval_queries = {}
                    if users_key not in cache:
                        if len(cache) >= 4:                    # bound the number of live evaluation graphs: drop the oldest query
                            old_q = cache.pop(next(iter(cache)))   # AND the graph / lists / workspace FusedStep keeps for it
                            fused.drop_eval_graph(old_q)
                        cache[users_key] = torch.from_numpy(users_np.copy()).to(device)
                    q = cache[users_key]
                    if getattr(self, "_eval_own_list", None) is users_to_test:
                        self._eval_own = (users_to_test, len(users_to_test), q)
                st = data_generator.device_state(device)
                Ks_ = eval(args.Ks)
                if USE_GRAPH() and os.environ.get("LLMREC_EVAL_GRAPH", "1") == "1":
                    # ONE graph replay: forward, scoring, masked top-K AND the metrics (llmrec_topk_eval_sums: hits, per-user values and their
                    # sums, the twelve doubles written into pinned host memory by the graph's last launch): no launch, no copy behind it
                    # (--test_flag full: the same graph also ends with the full-rank AUC sweep, llmrec_score_auc_f32, and its sum)
                    full = args.test_flag != 'part'
                    fused.eval_topk(q, st["train"], max(Ks_), use_graph=True, held=st["val"] if is_val else st["test"], Ks=Ks_, auc=full)
                    sums = fused.eval_sums().numpy() / len(users_to_test)
                    auc = float(fused.eval_auc_sum()[0]) / len(users_to_test) if full else 0.
                    return {'precision': sums[0].copy(), 'recall': sums[1].copy(), 'ndcg': sums[2].copy(), 'hit_ratio': sums[3].copy(), 'auc': auc}
                idx, _ = fused.eval_topk(q, st["train"], max(Ks_), use_graph=False)
                if args.test_flag != 'part':
                    return test_full_on_device(fused.E_u, fused.E_i, users_to_test, is_val, topk=(q, idx))
                return test_torch(fused.E_u, fused.E_i, users_to_test, is_val, topk=(q, idx))
            ua_embeddings, ia_embeddings, *rest = self.model_mm(self.ui_graph, self.iu_graph, self.image_ui_graph,
                                                                self.image_iu_graph, self.text_ui_graph, self.text_iu_graph)
        if args.test_flag != 'part':
            return test_full_on_device(ua_embeddings, ia_embeddings, users_to_test, is_val)
        return test_torch(ua_embeddings, ia_embeddings, users_to_test, is_val)

    # -- one step ---------------------------------------------------------------------------------
    def _sample_host(self):
        """The reference's batch on the host (utility/load_data.py + main.py:213-224, same two RNG streams): users / pos / neg lists and the
        LLM-augmented triples as int64 arrays (random.sample over the batch's users, then the dictionary look-ups and the `< n_items` filter
        as array operations)."""
        users, pos_items, neg_items = data_generator.sample()
        users_aug = np.asarray(data_generator.py_sample(users, int(len(users) * args.aug_sample_rate)), dtype=np.int64)   # = random.sample(users, k)
        ap, an = self._aug_arrays()
        pos_aug, neg_aug = ap[users_aug], an[users_aug]
        ok = (pos_aug < self.n_items) & (neg_aug < self.n_items)
        users_aug, pos_aug, neg_aug = users_aug[ok], pos_aug[ok], neg_aug[ok]
        self.new_batch_size = int(users_aug.size)
        return users, pos_items, neg_items, users_aug, pos_aug, neg_aug

    def _pinned_pair(self, slots):
        """Two pinned int64 staging buffers used alternately; a buffer is reused only after the copy that read it has finished."""
        st = getattr(self, "_stage", None)
        if st is None or st["cap"] < slots:
            # zero-filled once: train_step_packed copies the WHOLE 3 b_max + 1 block, so the slots past the batch must hold valid ids (0), never
            # uninitialised host memory - today's kernels bound on n_valid, a future one reading B_cap entries must not gather out of range
            pins = [torch.zeros(slots, dtype=torch.int64).pin_memory() for _ in range(2)]
            st = self._stage = {"cap": slots, "pin": pins, "np": [p_.numpy() for p_ in pins], "dev": [None, None], "busy": [None, None], "i": 0}
        i = st["i"]; st["i"] = 1 - i
        if st["busy"][i] is not None:
            st["busy"][i].synchronize()
        return st, i

    def sample_batch(self):
        """(users, pos, neg) int64 device tensors incl. the LLM-augmented triples (main.py:213-224). On the GPU the three tensors are views
        of one of TWO alternating device staging buffers (like the pinned ones): a batch stays intact across ONE further sample_batch() call;
        the call after that overwrites it (in stream order)."""
        if self._device_sampler:
            u, p, n = data_generator.sample_device(args.seed, self._global_step, device)
            users = u.tolist()
            users_aug = np.asarray(random.sample(users, int(len(users) * args.aug_sample_rate)), dtype=np.int64)
            ap, an = self._aug_arrays()
            pos_aug, neg_aug = ap[users_aug], an[users_aug]
            ok = (pos_aug < self.n_items) & (neg_aug < self.n_items)
            users_aug, pos_aug, neg_aug = users_aug[ok], pos_aug[ok], neg_aug[ok]
            self.new_batch_size = int(users_aug.size)
            extra = torch.from_numpy(np.stack([users_aug, pos_aug, neg_aug])).to(device)
            return torch.cat([u, extra[0]]), torch.cat([p, extra[1]]), torch.cat([n, extra[2]])
        users, pos_items, neg_items, users_aug, pos_aug, neg_aug = self._sample_host()
        B, k = len(users), int(users_aug.size)
        n = B + k
        if device.type != "cuda":
            packed = np.empty((3, n), dtype=np.int64)
            packed[0, :B], packed[1, :B], packed[2, :B] = users, pos_items, neg_items
            packed[0, B:], packed[1, B:], packed[2, B:] = users_aug, pos_aug, neg_aug
            packed = torch.from_numpy(packed).to(device)
            return packed[0], packed[1], packed[2]
        # one ASYNCHRONOUS H2D copy per batch from one of two pinned staging buffers: a pageable copy would make the host wait for the
        # previous step's graph, i.e. serialise sampling and the GPU step (an epoch was 0.58 ms per step for a 0.46 ms step)
        st, i = self._pinned_pair(3 * (self.batch_size + int(self.batch_size * args.aug_sample_rate) + 64))
        if st["dev"][i] is None or st["dev"][i].numel() < st["cap"]:
            st["dev"][i] = torch.zeros(st["cap"], dtype=torch.int64, device=device)
        buf, dev = st["np"][i], st["dev"][i]
        buf[0:B], buf[n:n + B], buf[2 * n:2 * n + B] = users, pos_items, neg_items
        buf[B:n], buf[n + B:2 * n], buf[2 * n + B:3 * n] = users_aug, pos_aug, neg_aug
        dev[:3 * n].copy_(st["pin"][i][:3 * n], non_blocking=True)
        ev = torch.cuda.Event(); ev.record(); st["busy"][i] = ev
        return dev[0:n], dev[n:2 * n], dev[2 * n:3 * n]

    def train_step_packed(self):
        """Default mode, steady state: the host-sampled batch is written in the captured step's own layout into pinned memory and the step is
        ONE asynchronous H2D copy + ONE graph replay (FusedStep.step_packed)."""
        fused = self._fused_step()
        t0 = time()
        users, pos_items, neg_items, users_aug, pos_aug, neg_aug = self._sample_host()
        t_sample = time() - t0
        slots, b = fused.packed_layout()
        B, k = len(users), int(users_aug.size)
        if B + k > b:
            raise RuntimeError("train_step_packed: batch of %d exceeds the captured capacity %d" % (B + k, b))
        st, i = self._pinned_pair(max(slots, 3 * (b + 64)))
        buf = st["np"][i]
        buf[0:B], buf[b:b + B], buf[2 * b:2 * b + B] = users, pos_items, neg_items
        buf[B:B + k], buf[b + B:b + B + k], buf[2 * b + B:2 * b + B + k] = users_aug, pos_aug, neg_aug
        last = st.setdefault("filled", [0, 0])
        if B + k < last[i]:                                   # a shorter batch than this buffer's previous one: the stale tail goes back to id 0
            buf[B + k:last[i]] = 0; buf[b + B + k:b + last[i]] = 0; buf[2 * b + B + k:2 * b + last[i]] = 0
        last[i] = B + k
        buf[3 * b] = B + k
        self.model_mm.train()
        fused.step_packed(st["pin"][i][:slots])
        ev = torch.cuda.Event(); ev.record(); st["busy"][i] = ev
        self._global_step += 1
        return t_sample

    def _aug_arrays(self):
        """augmented_sample_dict as two int64 arrays indexed by user (a user without an entry gets ids past every item: filtered)."""
        if getattr(self, "_aug_np", None) is None:
            big = np.iinfo(np.int64).max
            ap = np.full(self.n_users, big, dtype=np.int64); an = np.full(self.n_users, big, dtype=np.int64)
            for u_, pair in self.augmented_sample_dict.items():
                if 0 <= int(u_) < self.n_users:
                    ap[int(u_)], an[int(u_)] = int(pair[0]), int(pair[1])
            self._aug_np = (ap, an)
        return self._aug_np

    def _fused_step(self):
        """The fused step (llmrec_amd/fused.py) when the configuration allows it: no dropout, no
        --mask. LLMREC_FUSED=0 forces the modular autograd path; LLMREC_GRAPH=0 issues the fused step's
        launches one by one instead of replaying the captured HIP graph. LLMREC_FUSED_DROPOUT=1 (opt-in) keeps
        --drop_rate > 0 in the fused step: the masks are then the library's counter-based stream of
        (--seed, step, tensor, row, column), not torch's. LLMREC_FUSED=mask (opt-in) keeps --mask / --mask_rate > 0 in the fused step:
        the masked rows are then the library's lists of (--seed, round, side), not torch.randperm's (step_options.route names what
        still leaves it)."""
        if self._fused is None:
            # the reference masks user features whenever mask_rate > 0, with or without --mask (Models.py:139-142):
            # the fused path reads the unmasked features, so any of the three sends the step down the modular path
            # the fused step's eight-problem loss launches stage the batch in LDS (LLMREC_BPR_MAX_B); a larger batch trains on the
            # modular path, whose ops.bpr_prune selects with the multi-block kernels - or, under LLMREC_FUSED=wide (opt-in), in the
            # fused step's wide loss segment (FusedStep.WIDE_FROM). The predicate: step_options.route
            from llmrec_amd import step_options
            b_max = self.batch_size + int(self.batch_size * args.aug_sample_rate)
            path = step_options.route(os.environ.get("LLMREC_FUSED"), os.environ.get("LLMREC_FUSED_DROPOUT"), mask=args.mask,
                                      mask_rate=args.mask_rate, drop_rate=args.drop_rate, b_max=b_max,
                                      cap=ops.CONST["LLMREC_BPR_MAX_B"], wide_cap=ops.CONST["LLMREC_BPR_WIDE_MAX_B"],
                                      n_users=self.n_users, n_items=self.n_items)
            self._route = path if device.type == "cuda" else "modular"   # (checkpoints record it)
            if path != "modular" and device.type == "cuda":
                from llmrec_amd.fused import FusedStep
                graph = type("G", (), {"ui": ops.operand_from_sparse_tensor(self.ui_graph),
                                       "iu": ops.operand_from_sparse_tensor(self.iu_graph)})
                drop = dict(drop_rate=args.drop_rate, drop_seed=args.seed) if args.drop_rate != 0 else {}
                if args.mask or args.mask_rate != 0:             # (LLMREC_FUSED=mask: route() keeps no other value here)
                    drop = dict(mask_rate=args.mask_rate, mask_items=bool(args.mask), mask_seed=args.seed)
                    if args.mask:
                        drop.update(decoder=self.decoder, user_targets=self.user_init_embedding, item_targets=self.item_attribute_embedding,
                                    att_re_rate=args.att_re_rate, feat_loss_type="mse" if args.feat_loss_type == "mse" else "sce", alpha_l=args.alpha_l)
                self._fused = FusedStep(self.model_mm, graph, self.hyper,
                                        (args.model_cat_rate, args.user_cat_rate, args.item_cat_rate), self.optimizer, b_max, **drop)
            else:
                self._fused = False
        return self._fused

    def _device_batcher(self):
        """engine.DeviceBatcher over the training CSR and the augmented_sample_dict (LLMREC_DEVICE_SAMPLER=1)."""
        if getattr(self, "_batcher", None) is None:
            st = data_generator.device_state(device)
            ap, an = self._aug_arrays()
            self._batcher = engine.DeviceBatcher(st["train"], st["exist_users"], self.n_items, self.batch_size,
                                                 torch.from_numpy(ap).to(device), torch.from_numpy(an).to(device),
                                                 args.aug_sample_rate, args.seed)
        return self._batcher

    def train_step_sampled(self):
        """LLMREC_DEVICE_SAMPLER=1 + LLMREC_GRAPH=1: sampler, forward, the 8 losses, backward and AdamW are ONE
        HIP-graph replay (the sampler's step counter lives on the device); nothing else is enqueued per step."""
        fused = self._fused_step()
        self.model_mm.train()
        if fused.graph_exec is None:
            fused.capture(batcher=self._device_batcher())        # the capture's warm-up is a real step
            out = (fused.scal[1].clone(), fused.scal[2].clone(), fused.scal[3].clone())
        else:
            out = tuple(x.clone() for x in fused.step())
        self._global_step += 1
        return out

    def train_epoch_sampled(self, n_batch: int):
        """n_batch steps of the in-graph-sampler path as graph replays only; returns the device sums [loss, mf, emb] (float64)."""
        fused = self._fused_step()
        self.model_mm.train()
        fused.epoch_sums.zero_()
        todo = n_batch
        if fused.graph_exec is None or getattr(fused, "graph_multi", None) is None:
            fused.capture(batcher=self._device_batcher(), unroll=4)      # the capture's warm-up is a real step (and is summed)
            todo -= 1
        fused.run_steps(todo)
        self._global_step += n_batch
        return fused.epoch_sums.clone()

    def train_step(self, users, pos_items, neg_items, n_valid=None, clone=True):
        """Forward, the 8 BPR(+prune) losses, feature regulariser, backward, AdamW.
        Returns the device scalars (batch_loss, mf_loss, emb_loss); clone=False: views of the step's own buffer (the epoch loop reads
        the running sums the step keeps on the device instead)."""
        fused = self._fused_step()
        if fused:
            self.model_mm.train()
            if USE_GRAPH() and fused.graph_exec is None:
                fused.capture(users, pos_items, neg_items, n_valid)      # the capture run itself is a real step
                out = (fused.scal[1], fused.scal[2], fused.scal[3])
            else:
                out = fused.step(users, pos_items, neg_items, n_valid)
            if clone:
                out = tuple(x.clone() for x in out)
            if self._on_bpr is not None:
                for k in range(fused.n_prob):
                    self._on_bpr(fused.out[k, 0].clone(), fused.out[k, 1].clone())
            self._global_step += 1
            return out
        out = engine.train_step(self.model_mm, self.optimizer, self.ui_graph, self.iu_graph, users, pos_items, neg_items,
                                self.hyper, n_valid=n_valid, on_bpr=self._on_bpr,
                                extra_loss=self._mask_loss if args.mask else None)
        # (the reference calls clip_grad_norm_ before zero_grad(), on gradients that are then
        #  discarded, main.py:274-275 - it has no effect on the update and is omitted)
        self._global_step += 1
        return out

    def _mask_loss(self, fw):
        """Attribute-restoration term (reference main.py:258-271); off unless --mask."""
        user_prof_feat, item_att_feats, i_mask_nodes, u_mask_nodes = fw[8], fw[11], fw[12], fw[13]
        input_i = {value: item_att_feats[value][i_mask_nodes] for value in item_att_feats.keys()}
        # the reference wraps the user input in torch.tensor(...) (main.py:262), which detaches it
        decoded_u, decoded_i = self.decoder(user_prof_feat[u_mask_nodes].detach(), input_i)
        crit = self.mse_criterion if args.feat_loss_type == 'mse' else self.sce_criterion
        loss = crit(decoded_u, torch.as_tensor(self.user_init_embedding[u_mask_nodes]).float().to(device), alpha=args.alpha_l)
        for index, value in enumerate(item_att_feats.keys()):
            target = torch.as_tensor(self.item_attribute_embedding[value][i_mask_nodes]).float().to(device)
            loss = loss + crit(decoded_i[index], target, alpha=args.alpha_l)
        return args.att_re_rate * loss

    # -- checkpoints (llmrec_amd/checkpoint.py; opt-in: LLMREC_CHECKPOINT / LLMREC_CHECKPOINT_EVERY / LLMREC_RESUME) -----------------
    def _checkpointer(self):
        """The run's Checkpointer over the owners of its device state: the fused step (parameters, AdamW, its counters and stamps), the
        in-graph sampler where there is one, and the decoder; on the per-op path the parameters and FusedAdamW's state (its dropout is
        covered by torch's generator state). --mask / --mask_rate > 0 on the per-op path is refused: that path rewrites the feature
        matrices through torch.randperm every forward, and nothing here saves or replays them."""
        if getattr(self, "_ckpt", None) is None:
            from llmrec_amd import checkpoint, step_options
            fused = self._fused_step()
            if not fused and (args.mask or args.mask_rate != 0):
                raise RuntimeError("checkpoints of --mask / --mask_rate > 0 need the fused step (LLMREC_FUSED=mask): the per-op path's "
                                   "masked feature matrices are not part of a checkpoint")
            in_graph_sampler = bool(self._device_sampler and USE_GRAPH() and fused)
            listed = lambda fn: type("Listed", (), {"state_tensors": staticmethod(fn)})()
            parts = [fused] if fused else [listed(lambda: engine.model_state_tensors(self.model_mm, self.optimizer))]
            if in_graph_sampler:
                parts.append(self._device_batcher())
            if not (fused and fused.restore):                   # (a restoring step lists the decoder itself)
                parts.append(listed(lambda: [("decoder/" + n, p_.data) for n, p_ in self.decoder.named_parameters()]))
            csr = self.ui_graph_raw.tocsr().copy()
            csr.sort_indices()
            describe = {
                "route": self._route, "device_sampler": bool(self._device_sampler),
                "step_options": {f: getattr(fused, f) for f in step_options.StepOptions._fields} if fused else None,
                "fingerprint": checkpoint.fingerprint(vars(args), self.n_users, self.n_items, csr.nnz, csr.indptr.astype(np.int64),
                                                      csr.indices.astype(np.int64))}
            self._ckpt = checkpoint.Checkpointer(parts, os.environ.get("LLMREC_CHECKPOINT") or None, describe, log=self.logger.logging)
        return self._ckpt

    def _checkpoint_host(self, **more):
        return dict({"_global_step": self._global_step}, **more)

    def save_checkpoint(self, path, **host_state):
        """The state at this step boundary as one file (any step boundary; train() itself saves at epoch ends). Blocks until it is in place."""
        self._checkpointer().save(os.path.abspath(path), self._checkpoint_host(**host_state))

    def load_checkpoint(self, path, strict=True):
        """Make this trainer's state the file's - parameters, optimiser, the step's device counters, the host generators - and return the
        saved host state. Before the first step, or into a live captured step (a rollback). strict=False: a configuration mismatch warns."""
        host = self._checkpointer().load(path, strict=strict)
        self._global_step = int(host.get("_global_step", self._global_step))
        return host

    def train(self):
        now_time = datetime.now()
        run_time = datetime.strftime(now_time, '%Y_%m_%d__%H_%M_%S')
        training_time_list = []
        stopping_step = 0
        best_recall = 0
        test_ret = None
        in_graph_sampler = bool(self._device_sampler and USE_GRAPH() and self._fused_step())
        # the reference rebuilds this list every epoch (main.py:297); the test set does not change during training, so it is built once and the
        # evaluation recognises the object (its device query tensor is converted once, not 13 k python ints per epoch)
        users_to_test = list(data_generator.test_set.keys())
        self._eval_own_list, self._eval_own = users_to_test, None
        ckpt_dir, resume = os.environ.get("LLMREC_CHECKPOINT"), os.environ.get("LLMREC_RESUME")
        ckpt_every = int(os.environ.get("LLMREC_CHECKPOINT_EVERY", "0") or 0)
        first_epoch = last_epoch = 0
        if resume:                                                       # before the first step and before any capture
            host = self.load_checkpoint(resume)
            # (a file of save_checkpoint() without these keys resumes the state and starts the epoch count over)
            first_epoch, best_recall, stopping_step = int(host.get("epoch", -1)) + 1, host.get("best_recall", 0), int(host.get("stopping_step", 0))
            test_ret = host.get("test_ret")
            if test_ret is not None:
                test_ret = {k: np.array(v) if isinstance(v, list) else v for k, v in test_ret.items()}
            last_epoch = first_epoch - 1
            self.logger.logging("checkpoint: resumed %s, continuing at epoch %d" % (resume, first_epoch))
        if ckpt_dir:
            os.makedirs(ckpt_dir, exist_ok=True)
        # a request is taken behind the epoch's evaluation(s): an evaluation's masking round is inside the saved counter
        request = lambda name, ep: self._checkpointer().request(name, self._checkpoint_host(
            epoch=ep, best_recall=best_recall, stopping_step=stopping_step, test_ret=test_ret))
        for epoch in range(first_epoch, args.epoch):
            last_epoch = epoch
            t1 = time()
            n_batch = data_generator.n_train // args.batch_size + 1
            sums = torch.zeros(3, dtype=torch.float64, device=device)
            sample_time = 0.
            if in_graph_sampler:
                # sampler, forward, losses, backward and AdamW are graph replays (four steps per hipGraphLaunch); the three logged scalars
                # are summed in double inside the graph (llmrec_loss_assemble_f32): nothing else is enqueued between the replays
                sums = self.train_epoch_sampled(n_batch)
            else:
                fused = self._fused_step()
                if fused:
                    fused.epoch_sums.zero_()                             # the fused step sums the three logged scalars on the device (double)
                packed_ok = bool(fused) and USE_GRAPH() and not self._device_sampler and self._on_bpr is None and device.type == "cuda"
                for idx in _progress(range(n_batch)):
                    if packed_ok and fused.graph_exec is not None and getattr(fused, "batcher", None) is None:
                        sample_time += self.train_step_packed()          # sampling + one H2D copy + one graph replay
                        continue
                    sample_t1 = time()
                    users, pos_items, neg_items = self.sample_batch()
                    sample_time += time() - sample_t1
                    parts = self.train_step(users, pos_items, neg_items, clone=not fused)
                    if not fused:
                        sums += torch.stack(parts).double()
                if fused:
                    sums = fused.epoch_sums
            self.sample_time = sample_time                               # host seconds of this epoch spent in Data.sample() + the aug triples
            loss, mf_loss, emb_loss = (float(x) for x in sums.cpu())     # one sync per epoch
            fused_ = self._fused_step()
            if fused_ and hasattr(fused_, "check_wgrad_geometry"):       # (the host is synchronised here anyway: one more scalar read-back)
                fused_.check_wgrad_geometry()
            reg_loss, contrastive_loss = 0., 0.

            if math.isnan(loss):
                self.logger.logging('ERROR: loss is nan.')
                sys.exit()

            if (epoch + 1) % args.verbose != 0:
                perf_str = 'Epoch %d [%.1fs]: train==[%.5f=%.5f + %.5f + %.5f  + %.5f]' % (
                    epoch, time() - t1, loss, mf_loss, emb_loss, reg_loss, contrastive_loss)
                training_time_list.append(time() - t1)
                self.logger.logging(perf_str)

            t2 = time()
            ret = self.test(users_to_test, is_val=False)
            training_time_list.append(t2 - t1)
            t3 = time()

            if args.verbose > 0:
                perf_str = 'Epoch %d [%.1fs + %.1fs]: train==[%.5f=%.5f + %.5f + %.5f], recall=[%.5f, %.5f, %.5f, %.5f], ' \
                           'precision=[%.5f, %.5f, %.5f, %.5f], hit=[%.5f, %.5f, %.5f, %.5f], ndcg=[%.5f, %.5f, %.5f, %.5f]' % \
                           (epoch, t2 - t1, t3 - t2, loss, mf_loss, emb_loss, reg_loss,
                            ret['recall'][0], ret['recall'][1], ret['recall'][2], ret['recall'][-1],
                            ret['precision'][0], ret['precision'][1], ret['precision'][2], ret['precision'][-1],
                            ret['hit_ratio'][0], ret['hit_ratio'][1], ret['hit_ratio'][2], ret['hit_ratio'][-1],
                            ret['ndcg'][0], ret['ndcg'][1], ret['ndcg'][2], ret['ndcg'][-1])
                self.logger.logging(perf_str)
            if self._on_epoch is not None:
                self._on_epoch(epoch, loss, mf_loss, emb_loss, ret, (t2 - t1, t3 - t2))

            if ret['recall'][1] > best_recall:
                best_recall = ret['recall'][1]
                test_ret = self.test(users_to_test, is_val=False)
                self.logger.logging("Test_Recall@%d: %.5f,  precision=[%.5f], ndcg=[%.5f]" % (
                    eval(args.Ks)[1], test_ret['recall'][1], test_ret['precision'][1], test_ret['ndcg'][1]))
                stopping_step = 0
                if ckpt_dir:
                    request("best.ckpt", epoch)
            elif stopping_step < args.early_stopping_patience:
                stopping_step += 1
                self.logger.logging('#####Early stopping steps: %d #####' % stopping_step)
            else:
                self.logger.logging('#####Early stop! #####')
                break
            if ckpt_dir and ckpt_every > 0 and (epoch + 1) % ckpt_every == 0:
                request("last.ckpt", epoch)
        if ckpt_dir:                                                     # once, by early stop or by the epoch limit; in place on return
            request("last.ckpt", last_epoch)
            self._checkpointer().wait()
        self.logger.logging(str(test_ret))
        return best_recall, run_time


def set_seed(seed):
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


if __name__ == '__main__':
    set_seed(args.seed)
    config = dict()
    config['n_users'] = data_generator.n_users
    config['n_items'] = data_generator.n_items
    trainer = Trainer(data_config=config)
    trainer.train()
