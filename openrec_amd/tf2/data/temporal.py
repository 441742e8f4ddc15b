"""Batches of (history, next item) for the history-pooled recommenders (recommenders.VanillaYouTubeRec), by the rule of the
reference's tf1 TemporalSampler / TemporalEvaluationSampler, as vectorised NumPy generators:

  training    the user is drawn uniformly among users with at least 2 records, predict_pos uniformly in [1, len - 1]; the label
              is the user's item at predict_pos and the history the up-to-max_seq_len items before it;
  evaluation  every user with at least 2 records once: the label is the last item, the history the up-to-max_seq_len items before it.

A user's items stand in record order (the order of `raw`), or ascending by `time_field` (ties in record order).  Histories are
padded with zeros to max_seq_len, as the reference pads them; seq_len says how much of a row counts.  The draws come from
numpy.random.default_rng(seed): the rule is the reference's, its `random` stream is NOT reproduced bit for bit."""
import numpy as np


def _user_lists(raw, total_users, time_field):
    """-> (ptr int64 [total_users + 1], items int32 [records]) with every user's items in record / time order"""
    users = np.asarray(raw["user_id"], np.int64)
    items = np.asarray(raw["item_id"], np.int64)
    if users.size and (users.min() < 0 or users.max() >= total_users):
        raise IndexError(f"temporal batches: a user id outside [0, {total_users})")
    if time_field is None:
        order = np.argsort(users, kind="stable")
    else:
        order = np.lexsort((np.arange(users.size), np.asarray(raw[time_field]), users))
    ptr = np.zeros(int(total_users) + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(users, minlength=int(total_users)))
    return ptr, items[order].astype(np.int32)


def _gather(ptr, items, users, pos, max_seq_len):
    """histories that end before position pos[k] of users[k] -> seq [B, L] zero-padded, seq_len [B], label [B]"""
    L = int(max_seq_len)
    start = np.maximum(pos - L, 0)
    seq_len = (pos - start).astype(np.int32)
    t = np.arange(L)[None, :]
    live = t < seq_len[:, None]
    at = ptr[users][:, None] + start[:, None] + np.where(live, t, 0)
    seq = np.where(live, items[at], 0).astype(np.int32)
    return seq, seq_len, items[ptr[users] + pos].astype(np.int32)


def temporal_batches(raw, total_users, batch_size, max_seq_len, seed, time_field=None):
    """An endless generator of dicts(seq_item_id int32 [B, max_seq_len], seq_len int32 [B], label int32 [B], user_id int32 [B])."""
    if int(batch_size) < 1 or int(max_seq_len) < 1:
        raise ValueError(f"temporal_batches: batch_size = {batch_size}, max_seq_len = {max_seq_len}; both at least 1")
    ptr, items = _user_lists(raw, total_users, time_field)
    lens = np.diff(ptr)
    warm = np.flatnonzero(lens >= 2)
    if warm.size == 0:
        raise ValueError("temporal_batches: no user has two records")
    rng = np.random.default_rng(seed)
    while True:
        users = warm[rng.integers(0, warm.size, int(batch_size))]
        pos = rng.integers(1, lens[users])                       # uniform in [1, len - 1]
        seq, seq_len, label = _gather(ptr, items, users, pos, max_seq_len)
        yield dict(seq_item_id=seq, seq_len=seq_len, label=label, user_id=users.astype(np.int32))


def temporal_evaluation(raw, total_users, max_seq_len, time_field=None, batch_size=None):
    """A generator over the users with at least 2 records, in id order, of dicts like temporal_batches': the label is the user's
    last item.  batch_size None: one batch with all of them."""
    if int(max_seq_len) < 1:
        raise ValueError(f"temporal_evaluation: max_seq_len = {max_seq_len}; at least 1")
    ptr, items = _user_lists(raw, total_users, time_field)
    lens = np.diff(ptr)
    warm = np.flatnonzero(lens >= 2)
    step = warm.size if batch_size is None else int(batch_size)
    for k in range(0, warm.size, max(step, 1)):
        users = warm[k:k + step]
        seq, seq_len, label = _gather(ptr, items, users, lens[users] - 1, max_seq_len)
        yield dict(seq_item_id=seq, seq_len=seq_len, label=label, user_id=users.astype(np.int32))
