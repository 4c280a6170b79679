"""What the evaluation keys of a config mean -- config['metrics'], config['eval_args']['mode'], config['eval_route'] -- resolved and refused
before anything is built.  Package level: the evaluation loaders (data.dataloader.eval_loader_for) read the mode without loading the trainer.
"""
DEFAULT_METRICS = ('recall', 'hit', 'precision', 'mrr', 'ndcg')     # what evaluate returned before config['metrics'] was read
TOPK_METRICS = ('recall', 'mrr', 'ndcg', 'hit', 'precision', 'map')  # keys name@k
VALUE_METRICS = ('auc', 'mae', 'rmse', 'logloss')
# recbole's non-accuracy metrics (keys name@k): the only ones that need to know WHICH items are in the lists, so they are answered by the
# list route alone -- the lists of the mask + top-k kernels (k <= 1024) folded on the device by functional.ListStats, batch after batch --
# and they need the training set's item counts over the evaluated loader's column space: config['item_counts'] (data.train_item_counts of
# the target domain's training pairs), or the loader's own ``item_counts`` attribute.  tailpercentage reads config['tail_ratio'] (0.1).
NON_ACCURACY_METRICS = ('itemcoverage', 'averagepopularity', 'shannonentropy', 'giniindex', 'tailpercentage')
FUSED_TOPK_MAX = 64                   # the fused mask + top-k kernels keep a list in one wave: k <= 64
WIDE_TOPK_MAX = 1024                  # the wide mask + top-k behind them (model.full_sort_topk_wide): k <= 1024


def resolve_metrics(config):
    """config['metrics'] as recbole reads it (a name or a list of names, any letter case) -> tuple of lower-case names, or None when the
    key is absent (evaluate then returns what it always did).  Refused here, before anything is built: recbole's value metrics (they need
    the labeled evaluation mode), its non-accuracy metrics unless config['item_counts'] is given (they need the training set's item
    counts), unknown names."""
    if 'metrics' not in config or config['metrics'] is None:
        return None
    names = config['metrics']
    names = [names] if isinstance(names, str) else list(names)
    out = []
    for n in names:
        m = str(n).lower()
        if m in VALUE_METRICS:
            raise ValueError(f"metrics: {n!r} is a value metric: it needs recbole's labeled evaluation mode, which this trainer does not "
                             f"have (full-sort ranking only)")
        if m in NON_ACCURACY_METRICS and ('item_counts' not in config or config['item_counts'] is None):
            raise ValueError(f"metrics: {n!r} is a non-accuracy metric: it needs the training set's item counts, which evaluate() is not "
                             f"given: set config['item_counts'] (data.train_item_counts of the target domain's training pairs)")
        if m not in TOPK_METRICS and m not in NON_ACCURACY_METRICS and m != 'gauc':
            raise ValueError(f"metrics: unknown metric {n!r}; supported: {', '.join(TOPK_METRICS + NON_ACCURACY_METRICS)} (keys name@k) "
                             f"and gauc")
        if m not in out:
            out.append(m)
    if not out:
        raise ValueError('metrics: the list is empty')
    return tuple(out)


def resolve_eval_mode(config):
    """config['eval_args']['mode'] as recbole's ``Config._set_eval_neg_sample_args`` reads it -> (strategy, sample_by, distribution):
    absent or 'full' -> ('full', None, 'uniform'); 'uniN' -> ('by', N, 'uniform'); 'popN' -> ('by', N, 'popularity'), N a positive integer.
    Case-sensitive, as recbole is ('Uni5' is refused).  'labeled' and everything else raise ValueError, before anything is built."""
    args = config['eval_args'] if 'eval_args' in config and config['eval_args'] is not None else {}
    mode = args['mode'] if 'mode' in args and args['mode'] is not None else 'full'
    if mode == 'full':
        return 'full', None, 'uniform'
    if mode == 'labeled':
        raise ValueError("the mode [labeled] in eval_args is not provided: labeled evaluation and the value metrics (auc, mae, rmse, "
                         "logloss) need label-carrying evaluation data and training without negative sampling; use full, uniN or popN")
    if isinstance(mode, str) and mode[:3] in ('uni', 'pop') and mode[3:].isascii() and mode[3:].isdigit() and int(mode[3:]) > 0:
        return 'by', int(mode[3:]), 'uniform' if mode[:3] == 'uni' else 'popularity'
    raise ValueError(f'the mode [{mode}] in eval_args is not supported.')


def resolve_eval_route(config, metrics):
    """config['eval_route'] ('auto' | 'topk' | 'rank'): which of the two FULL-SORT routes a full-sort loader takes.  It does not concern a
    sampled-candidate loader (``eval_mode = 'sampled'``), which always ranks its positives inside the candidate lists."""
    route = config['eval_route'] if 'eval_route' in config and config['eval_route'] is not None else 'auto'
    if route not in ('auto', 'topk', 'rank'):
        raise ValueError(f"eval_route must be 'auto', 'topk' or 'rank', got {route!r}")
    if route == 'topk' and metrics is not None and 'gauc' in metrics:
        raise ValueError("eval_route='topk' cannot answer gauc: a top-k list does not hold the rank of every positive over the whole "
                         "catalogue; use eval_route='rank' or 'auto'")
    return route
