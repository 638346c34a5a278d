"""Recommend from a checkpoint: the top-K items for a list of users, optionally among an allow-list or outside a deny-list of items.

    python recommend.py --checkpoint ckpt/best.ckpt (--users users.txt | --histories hist.txt) --topk 20 [--allow_items F | --deny_items F]
                        [--include_seen] [--exclude F] [--candidates F] [--item_groups F --per_group M] --out out.npz --dataset netflix_valid_item --data_path ./data/ [the flags the model
                        was trained with ...]

The flags above are this script's own; EVERY OTHER argument goes to the drop-in's parser untouched (utility/parser.py - the
configuration the checkpoint was written under: a checkpoint of another configuration fails its fingerprint check). The script builds
the Trainer, loads the checkpoint, recommends (llmrec_amd.serve.Recommender) and writes out.npz with `users` int64 [n], `items` int64
[n, K] (-1 behind the last candidate) and `scores` float32 [n, K]. It trains nothing. Id files are .npy (integers) or text with one id
per line. --exclude: (user, item) pairs - a .npy integer array [m, 2] or text with one `user item` per line -, items left out for that user
on top of the train row; a pair applies to every occurrence of its user in --users, and a user that is not listed is ignored.
--histories (instead of --users): the users are NOT rows of the training graph - (row, item) pairs in the format of --exclude, row q the
q-th new user (rows 0 .. the largest row listed; a row without a pair has an empty history). Each is embedded from its item history by
the trained model with the item side held fixed (Recommender.recommend_new) and ranked as above; the history's own items are left out
unless --include_seen; --exclude pairs are then (row, item) too; the .npz holds `rows` int64 [n] in place of `users`.
--candidates: (user, item) pairs in the format of --exclude, (row, item) with --histories - each user's OWN candidate list: the script then
ranks only those items per user (Recommender.rank / rank_new; a user without a pair gets an empty list), and --topk has no 1024 cap.
--item_groups with --per_group (both or neither): quotas - a .npy integer array [n_items] or text with one group id per line, line i the
group of item i (negative: no group), and the cap M >= 1: a list then holds at most M items of any one group, taken greedily down the
user's ranking (exact; Recommender's group_of / per_group). They work with --users and --histories, with and without --candidates (under
quotas --topk <= 1024 on every route).
--mask / --mask_rate != 0 are refused: with them every forward is a masking round, and a serving run must not advance one."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))


def own_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, allow_abbrev=False)
    p.add_argument("--checkpoint", required=True, help="a file of Trainer.save_checkpoint / LLMREC_CHECKPOINT (best.ckpt, last.ckpt)")
    who = p.add_mutually_exclusive_group(required=True)
    who.add_argument("--users", help="user ids: .npy or text, one id per line")
    who.add_argument("--histories", help="new users as (row, item) pairs: .npy [m, 2] or text, one `row item` per line; row q is the q-th new user")
    p.add_argument("--topk", type=int, required=True, help="items per user (<= 1024)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--allow_items", help="rank only among these item ids (.npy or text)")
    g.add_argument("--deny_items", help="rank among all but these item ids (.npy or text)")
    p.add_argument("--include_seen", action="store_true", help="do not exclude the user's train items (--histories: the history's items)")
    p.add_argument("--exclude", help="(user, item) pairs to leave out per user: .npy [m, 2] or text, one `user item` per line")
    p.add_argument("--candidates", help="(user, item) pairs: rank only each user's own candidates; .npy [m, 2] or text, one `user item` per line")
    p.add_argument("--item_groups", help="quotas: the group id of every item, .npy [n_items] or text with one id per line (negative: no group)")
    p.add_argument("--per_group", type=int, help="quotas: at most this many items of any one group per list (>= 1); needs --item_groups")
    p.add_argument("--out", required=True, help="the .npz to write")
    return p


def split_argv(argv):
    """(this script's namespace, the arguments left for the drop-in's parser - in their order, untouched)."""
    p = own_parser()
    own, rest = p.parse_known_args(list(argv))
    if (own.item_groups is None) != (own.per_group is None):
        p.error("--item_groups and --per_group go together")
    if own.per_group is not None and own.per_group < 1:
        p.error("--per_group must be at least 1")
    return own, rest


def read_ids(path: str) -> np.ndarray:
    """int64 ids from a .npy file or from text with one id per line (blank lines ignored)."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.dtype.kind not in "iu":
            raise SystemExit("%s: integer ids expected, got %s" % (path, a.dtype))
        return a.reshape(-1).astype(np.int64)
    with open(path) as f:
        return np.asarray([int(line) for line in f if line.strip()], dtype=np.int64)


def read_pairs(path: str) -> np.ndarray:
    """int64 (user, item) pairs [m, 2] from a .npy file or from text with one `user item` per line (blank lines ignored)."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.dtype.kind not in "iu" or a.ndim != 2 or a.shape[1] != 2:
            raise SystemExit("%s: an integer array [m, 2] of (user, item) pairs expected, got %s %s" % (path, a.dtype, a.shape))
        return a.astype(np.int64)
    pairs = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            w = line.split()
            if not w:
                continue
            if len(w) != 2:
                raise SystemExit("%s:%d: `user item` expected, got %r" % (path, no, line.strip()))
            pairs.append((int(w[0]), int(w[1])))
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2)


def exclusion_lists(pairs: np.ndarray, users: np.ndarray) -> dict:
    """{user: int64 item ids, in file order} of the pairs whose user is listed - Recommender.recommend's dict form, which applies a list
    to every occurrence of its user."""
    listed = np.isin(pairs[:, 0], users)
    out = {}
    for u, i in pairs[listed]:
        out.setdefault(int(u), []).append(int(i))
    return {u: np.asarray(v, dtype=np.int64) for u, v in out.items()}


def refuse_masking(dropin_args):
    """A serving run must not advance a masking round (every forward of such a configuration is one)."""
    if dropin_args.mask or dropin_args.mask_rate != 0:
        raise SystemExit("recommend.py: --mask / --mask_rate != 0 are refused: every forward of a masking configuration is a masking round "
                         "(it redraws the masked rows and advances the round counter), and a serving run must not advance one. "
                         "Run with --mask_rate 0 and without --mask.")


def load_dropin(rest):
    """Import the drop-in (main.py) under the remaining arguments: four of its modules parse sys.argv at import."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    old = sys.argv
    sys.argv = ["main.py"] + list(rest)
    try:
        return importlib.import_module("main")
    finally:
        sys.argv = old


def main(argv=None):
    own, rest = split_argv(sys.argv[1:] if argv is None else argv)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from utility.parser import parse_args
    refuse_masking(parse_args(rest))                               # (unknown flags are the drop-in parser's errors, raised here)
    if own.histories:
        pairs = read_pairs(own.histories)
        if pairs.size and pairs[:, 0].min() < 0:
            raise SystemExit("%s: a negative row" % own.histories)
        users = np.arange(int(pairs[:, 0].max()) + 1 if pairs.size else 0, dtype=np.int64)
        histories = exclusion_lists(pairs, users)
    else:
        users = read_ids(own.users)
    allow = read_ids(own.allow_items) if own.allow_items else None
    deny = read_ids(own.deny_items) if own.deny_items else None
    exclude = exclusion_lists(read_pairs(own.exclude), users) if own.exclude else None
    candidates = exclusion_lists(read_pairs(own.candidates), users) if own.candidates else None
    quota = dict(group_of=read_ids(own.item_groups), per_group=own.per_group) if own.item_groups else {}
    m = load_dropin(rest)
    from llmrec_amd.serve import Recommender
    m.set_seed(m.args.seed)
    trainer = m.Trainer(data_config={})
    rec = Recommender.from_checkpoint(trainer, own.checkpoint, fold_in=bool(own.histories))
    if own.histories:
        histories = [histories.get(int(q), ()) for q in users]
        if candidates is not None:
            items, scores = rec.rank_new(histories, candidates, own.topk, allow_items=allow, deny_items=deny, exclude_history=not own.include_seen,
                                         exclude=exclude, **quota)
        else:
            items, scores = rec.recommend_new(histories, own.topk, allow_items=allow, deny_items=deny, exclude_history=not own.include_seen,
                                              exclude=exclude, **quota)
    elif candidates is not None:
        items, scores = rec.rank(users, candidates, own.topk, allow_items=allow, deny_items=deny, exclude_seen=not own.include_seen, exclude=exclude,
                                 **quota)
    else:
        items, scores = rec.recommend(users, own.topk, allow_items=allow, deny_items=deny, exclude_seen=not own.include_seen, exclude=exclude,
                                      **quota)
    out = own.out if own.out.endswith(".npz") else own.out + ".npz"
    np.savez(out, items=items.cpu().numpy(), scores=scores.cpu().numpy(), **{"rows" if own.histories else "users": users})
    print("recommend.py: %d users x top %d -> %s" % (len(users), own.topk, out))


if __name__ == "__main__":
    main()
