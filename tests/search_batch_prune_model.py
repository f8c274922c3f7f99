"""The contract of mlz_stream_search_batch_device_pruned (include/minlz_hip_search_batch_prune.h) in plain Python.  Per stream: the tables a
searcher finds (search_model.read_tables: uncompressed table chunks, 0x45, alone — a compressed one, 0x46, and one with a stale CRC count as no
table) and the union over the patterns of search_model.plan, which is every chunk with bytes once a pattern is not served.  Over the batch: the
class rule — the distinct configurations (T, M, B, field) of the healthy streams are numbered in descriptor order and only the first MAX_CLASSES
prune.  The results are search_batch_model.result's: a plan changes which chunks are decoded, never what is found."""
from tests import fold_model as FM
from tests import search_batch_model as BM
from tests import search_model as SMod

MAX_CLASSES = 4
result = BM.result


def served(cfg, B, patterns, fold=False):
    """The configuration gives every pattern a window (under folding: within the call's budget of variant hashes)."""
    if not fold:
        return all(SMod.checks(cfg, p, B) is not None for p in patterns)
    made = 0
    for p in patterns:
        chk = FM.checks(cfg, FM.fold(p), B)
        if chk is None or made + FM.n_hashes(chk) > FM.MAX_HASHES:
            return False
        made += FM.n_hashes(chk)
    return True


def stream_plan(stream, patterns, prunes=True, ignore_crc=False, fold=False):
    """One stream -> dict(plan: the data chunks decoded, sizes, whole: it holds bytes and is decoded whole because nothing prunes it,
    tabbed: its chunks with a usable table when it is pruned, cfg: (T, M, B, field) or None)."""
    cfg, B, tables = SMod.read_tables(stream, ignore_crc)
    sizes = [n for n, _ in SMod.data_grid(stream)]
    everything = [k for k in range(len(sizes)) if sizes[k]]
    key = None if cfg is None else (cfg[0], cfg[1], B, bytes(cfg[2]))
    if cfg is None or not prunes or not served(cfg, B, patterns, fold):
        return dict(plan=everything, sizes=sizes, whole=bool(everything), tabbed=0, cfg=key)
    if fold:
        plan = FM.plan_many([tables], sizes, [FM.fold(p) for p in patterns], [cfg], [B])[0]
    else:
        plan = sorted(set().union(*[SMod.plan(tables, sizes, p, cfg, B) for p in patterns]))
    return dict(plan=plan, sizes=sizes, whole=False, tabbed=sum(t is not None for t in tables), cfg=key)


def plan(streams, patterns, healthy=None, ignore_crc=False, fold=False):
    """streams: every stream's bytes; healthy[i] False: a stream with a framing error, of which nothing is planned or searched ->
    dict(plans: per stream the chunks decoded (None for an unhealthy one), decoded: their number, tabbed, skipped, classes, whole: stats 4 .. 7,
    pruning: per stream whether its class prunes)."""
    n = len(streams)
    healthy = [True] * n if healthy is None else healthy
    classes, pruning = [], []
    for s, ok in zip(streams, healthy):
        key = stream_plan(s, patterns, False)["cfg"] if ok else None
        if key is not None and key not in classes:
            classes.append(key)
        pruning.append(key is not None and classes.index(key) < MAX_CLASSES)
    per = [stream_plan(s, patterns, pr, ignore_crc, fold) if ok else None for s, ok, pr in zip(streams, healthy, pruning)]
    live = [p for p in per if p is not None]
    return dict(plans=[None if p is None else p["plan"] for p in per], sizes=[None if p is None else p["sizes"] for p in per],
                decoded=sum(len(p["plan"]) for p in live), tabbed=sum(p["tabbed"] for p in live),
                skipped=sum(1 for p in live if any(p["sizes"]) and not p["plan"]), classes=len(classes), whole=sum(1 for p in live if p["whole"]), pruning=pruning)
