"""What recbole's non-accuracy metrics take from the training set: ``dataset.item_counter`` as a count vector over the loader's column
space, and TailPercentage's tail set as a mask over it (recbole/evaluator/metrics.py ``TailPercentage.get_tail``, third-party)."""
import numpy as np
import torch


def train_item_counts(pairs, item_num, device='cpu'):
    """int64 [item_num]: how often each item id occurs in column 1 of the training (user, item) ``pairs`` (tensor or array [n, 2]) -- what
    recbole's ``dataset.item_counter`` holds.  Index 0 (PAD) stays 0.  An id outside [0, item_num) is refused."""
    pairs = pairs if torch.is_tensor(pairs) else torch.as_tensor(np.asarray(pairs))
    items = pairs.reshape(-1, 2)[:, 1].to(device=device, dtype=torch.int64)
    item_num = int(item_num)
    if items.numel() and (int(items.min()) < 0 or int(items.max()) >= item_num):
        raise ValueError(f'train_item_counts: item ids span [{int(items.min())}, {int(items.max())}], outside [0, {item_num})')
    counts = torch.bincount(items, minlength=item_num)
    counts[:1] = 0
    return counts


def tail_items(item_counts, tail_ratio=0.1):
    """bool [item_num]: recbole's tail set over the items the counter holds (count >= 1; an item never interacted with is in no tail).
    ``tail_ratio`` None or <= 0 means 0.1.  A ratio > 1 is a count threshold: the items with count <= ratio.  Otherwise the first
    max(int(n_seen * ratio), 1) items in the order (count ascending, item id ascending), from one stable sort."""
    ratio = 0.1 if tail_ratio is None or tail_ratio <= 0 else tail_ratio
    counts = torch.as_tensor(item_counts).to(torch.int64)
    seen = counts >= 1
    if ratio > 1:
        return seen & (counts <= ratio)
    n_seen = int(seen.sum())
    mask = torch.zeros_like(seen)
    if n_seen == 0:
        return mask
    # the unseen items sort behind every seen one; among equal counts a stable sort keeps the ids ascending
    order = torch.sort(torch.where(seen, counts, torch.full_like(counts, torch.iinfo(torch.int64).max)), stable=True).indices
    mask[order[:min(max(int(n_seen * ratio), 1), n_seen)]] = True
    return mask
