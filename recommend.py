"""Recommend from a checkpoint: the top-K items for a list of users, optionally among an allow-list or outside a deny-list of items.

    python recommend.py --checkpoint ckpt/best.ckpt --users users.txt --topk 20 [--allow_items F | --deny_items F] [--include_seen]
                        --out out.npz --dataset netflix_valid_item --data_path ./data/ [the flags the model was trained with ...]

The flags above are this script's own; EVERY OTHER argument goes to the drop-in's parser untouched (utility/parser.py - the
configuration the checkpoint was written under: a checkpoint of another configuration fails its fingerprint check). The script builds
the Trainer, loads the checkpoint, recommends (llmrec_amd.serve.Recommender) and writes out.npz with `users` int64 [n], `items` int64
[n, K] (-1 behind the last candidate) and `scores` float32 [n, K]. It trains nothing. Id files are .npy (integers) or text with one id
per line. --mask / --mask_rate != 0 are refused: with them every forward is a masking round, and a serving run must not advance one."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))


def own_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, allow_abbrev=False)
    p.add_argument("--checkpoint", required=True, help="a file of Trainer.save_checkpoint / LLMREC_CHECKPOINT (best.ckpt, last.ckpt)")
    p.add_argument("--users", required=True, help="user ids: .npy or text, one id per line")
    p.add_argument("--topk", type=int, required=True, help="items per user (<= 1024)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--allow_items", help="rank only among these item ids (.npy or text)")
    g.add_argument("--deny_items", help="rank among all but these item ids (.npy or text)")
    p.add_argument("--include_seen", action="store_true", help="do not exclude the user's train items")
    p.add_argument("--out", required=True, help="the .npz to write")
    return p


def split_argv(argv):
    """(this script's namespace, the arguments left for the drop-in's parser - in their order, untouched)."""
    return own_parser().parse_known_args(list(argv))


def read_ids(path: str) -> np.ndarray:
    """int64 ids from a .npy file or from text with one id per line (blank lines ignored)."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.dtype.kind not in "iu":
            raise SystemExit("%s: integer ids expected, got %s" % (path, a.dtype))
        return a.reshape(-1).astype(np.int64)
    with open(path) as f:
        return np.asarray([int(line) for line in f if line.strip()], dtype=np.int64)


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
    users = read_ids(own.users)
    allow = read_ids(own.allow_items) if own.allow_items else None
    deny = read_ids(own.deny_items) if own.deny_items else None
    m = load_dropin(rest)
    from llmrec_amd.serve import Recommender
    m.set_seed(m.args.seed)
    trainer = m.Trainer(data_config={})
    rec = Recommender.from_checkpoint(trainer, own.checkpoint)
    items, scores = rec.recommend(users, own.topk, allow_items=allow, deny_items=deny, exclude_seen=not own.include_seen)
    out = own.out if own.out.endswith(".npz") else own.out + ".npz"
    np.savez(out, users=users, items=items.cpu().numpy(), scores=scores.cpu().numpy())
    print("recommend.py: %d users x top %d -> %s" % (len(users), own.topk, out))


if __name__ == "__main__":
    main()
