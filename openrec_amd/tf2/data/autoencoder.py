"""Batches of (input bag, label set) for the autoencoder recommenders (recommenders.MultDAE; Liang et al. 2018), as vectorised
NumPy generators:

  training    the user is drawn uniformly among users with at least 1 record; the label set is the user's full item list (up to
              max_len items, in record order) and the input bag the same list with every entry dropped with probability
              `dropout`, independently, but at least one entry kept -- the denoising autoencoder's corrupted input;
  evaluation  every user with records in both parts once, in id order: the fold-in history is the user's items of raw_train,
              the positives the user's items of raw_heldout, the exclusion list the fold-in history itself.

Lists are padded with zeros on the right; the lengths say how much of a row counts.  The draws come from
numpy.random.default_rng(seed): the same seed gives the same batches."""
import numpy as np

from .temporal import _user_lists


def _padded(ptr, items, users, max_len):
    """the lists of `users` -> (rows [B, L] zero-padded, len [B]); L = the longest list, at most max_len"""
    lens = np.diff(ptr)[users]
    if max_len is not None:
        lens = np.minimum(lens, int(max_len))
    L = max(int(lens.max(initial=0)), 1)
    t = np.arange(L)[None, :]
    live = t < lens[:, None]
    rows = np.where(live, items[ptr[users][:, None] + np.where(live, t, 0)], 0).astype(np.int32)
    return rows, lens.astype(np.int32)


def autoencoder_batches(raw, total_users, batch_size, seed, dropout=0.5, max_len=None):
    """An endless generator of dicts(in_items int32 [B, L], in_len int32 [B], label_items int32 [B, L], label_len int32 [B],
    user_id int32 [B]); L is the longest label set of the batch."""
    if int(batch_size) < 1 or (max_len is not None and int(max_len) < 1):
        raise ValueError(f"autoencoder_batches: batch_size = {batch_size}, max_len = {max_len}; both at least 1")
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError(f"autoencoder_batches: dropout = {dropout} outside [0, 1)")
    ptr, items = _user_lists(raw, total_users, None)
    warm = np.flatnonzero(np.diff(ptr) >= 1)
    if warm.size == 0:
        raise ValueError("autoencoder_batches: no user has a record")
    rng = np.random.default_rng(seed)
    while True:
        users = warm[rng.integers(0, warm.size, int(batch_size))]
        lab, lab_len = _padded(ptr, items, users, max_len)
        B, L = lab.shape
        live = np.arange(L)[None, :] < lab_len[:, None]
        keep = live & (rng.random((B, L)) >= float(dropout))
        forced = np.minimum((rng.random(B) * lab_len).astype(np.int64), lab_len - 1)        # the entry kept where all were dropped
        none = ~keep.any(axis=1)
        keep[np.flatnonzero(none), forced[none]] = True
        order = np.argsort(~keep, axis=1, kind="stable")                                   # the kept entries first, in list order
        in_len = keep.sum(axis=1).astype(np.int32)
        in_items = np.where(np.arange(L)[None, :] < in_len[:, None], np.take_along_axis(lab, order, axis=1), 0).astype(np.int32)
        yield dict(in_items=in_items, in_len=in_len, label_items=lab, label_len=lab_len, user_id=users.astype(np.int32))


def autoencoder_evaluation(raw_train, raw_heldout, total_users, max_len=None, batch_size=None):
    """A generator over the users with at least one record in each part, in id order, of dicts(seq_item_id int32 [B, L],
    seq_len int32 [B], user_id int32 [B]) as temporal_evaluation gives them -- the fold-in history --, with
    pos_item_id int32 [B, Lp], pos_len int32 [B] (the held-out items) and excl_item_id, excl_len (the fold-in history: items
    never to be recommended back).  batch_size None: one batch with all of them."""
    ptr, items = _user_lists(raw_train, total_users, None)
    hptr, hitems = _user_lists(raw_heldout, total_users, None)
    warm = np.flatnonzero((np.diff(ptr) >= 1) & (np.diff(hptr) >= 1))
    step = warm.size if batch_size is None else int(batch_size)
    for k in range(0, warm.size, max(step, 1)):
        users = warm[k:k + step]
        seq, seq_len = _padded(ptr, items, users, max_len)
        pos, pos_len = _padded(hptr, hitems, users, None)
        yield dict(seq_item_id=seq, seq_len=seq_len, user_id=users.astype(np.int32), pos_item_id=pos, pos_len=pos_len,
                   excl_item_id=seq, excl_len=seq_len)
