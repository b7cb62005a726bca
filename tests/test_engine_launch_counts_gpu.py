"""Kernel launches of the LSTUR, NPA and NAML engines, counted by the library (ebn_launch_count): one eager training step,
one eval_loss, and the cached user-vector call of each engine.  These models have no benchmark: the counts are what pins
"the step launches what it launched" across host-side changes.  The literals were read off the commit BEFORE the engines
got their shared base (the same body run there), not off the code under test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, H, C, T, TB, E, F, A, WINDOW = 2, 3, 2, 5, 6, 8, 8, 4, 3
VOCAB, N_USERS, USER_DIM, N_CAT, CAT_DIM, DROPOUT, N_ROWS = 50, 5, 4, 3, 4, 0.2, 11
SEED = 5

KINDS = ("lstur_ini", "lstur_con", "npa", "naml_fused", "naml_unfused")

# kind: (one eager _train_kernels, eval_loss, the cached user-vector call) -- as counted on the pre-refactor engines
EXPECTED = {
    "lstur_ini": (34, 12, 4),     # pre-refactor: 34 / 12 / 4
    "lstur_con": (42, 15, 7),     # pre-refactor: 42 / 15 / 7  (the Dense of "con": 3 forward + 5 backward GEMMs)
    "npa": (37, 14, 8),           # pre-refactor: 37 / 14 / 8
    "naml_fused": (43, 16, 1),    # pre-refactor: 43 / 16 / 1  (score_cached(return_user=True) is NAML's cached user-vector call)
    "naml_unfused": (47, 16, 1),  # pre-refactor: 47 / 16 / 1  (the head as four launches instead of one)
}


def build_engine(kind):
    rng = np.random.default_rng(SEED)
    table = rng.uniform(-0.5, 0.5, (VOCAB, E)).astype(np.float32)
    common = dict(dropout=DROPOUT, learning_rate=1e-3, loss="cross_entropy_loss", seed=SEED)
    if kind.startswith("lstur"):
        from ebrec.models.newsrec._engine_lstur import LSTUREngine

        return LSTUREngine(table, N_USERS, T, H, F, WINDOW, A, F, kind[-3:], **common)
    if kind == "npa":
        from ebrec.models.newsrec._engine_npa import NPAEngine

        return NPAEngine(table, N_USERS, T, H, F, WINDOW, A, USER_DIM, **common)
    from ebrec.models.newsrec._engine_naml import NAMLEngine

    eng = NAMLEngine(table, T, TB, H, F, WINDOW, A, N_CAT, CAT_DIM, N_CAT, CAT_DIM, **common)
    eng.fuse_user_head = kind == "naml_fused"
    return eng


def batch(kind, seed=0):
    """(the train_step / eval_loss inputs before y, y) of one (B, C) batch."""
    rng = np.random.default_rng(100 + seed)
    y = np.zeros((B, C), np.float32)
    y[np.arange(B), rng.integers(0, C, B)] = 1
    tok = lambda n, L: rng.integers(1, VOCAB, (B, n, L))
    if kind.startswith("naml"):
        cat = lambda n: rng.integers(0, N_CAT, (B, n, 1))
        return (tok(H, T), tok(H, TB), cat(H), cat(H), tok(C, T), tok(C, TB), cat(C), cat(C)), y
    return (rng.integers(0, N_USERS + 1, (B, 1)), tok(H, T), tok(C, T)), y


def catalogue(kind, seed=0):
    """encode_catalogue() arguments of an N_ROWS-article catalogue, and (his_idx (B, H), cand_idx (B*C,), cand_imp (B*C,))."""
    rng = np.random.default_rng(200 + seed)
    title = rng.integers(1, VOCAB, (N_ROWS, T))
    idx = (rng.integers(0, N_ROWS, (B, H)), rng.integers(0, N_ROWS, B * C), np.repeat(np.arange(B), C))
    if kind.startswith("naml"):
        return (title, rng.integers(1, VOCAB, (N_ROWS, TB)), rng.integers(0, N_CAT, N_ROWS), rng.integers(0, N_CAT, N_ROWS)), idx
    return (title,), idx


def launch_counts(kind):
    import torch

    from ebrec import _hip

    count = lambda: int(_hip.lib().ebn_launch_count())
    eng = build_engine(kind)
    xs, y = batch(kind)
    if kind.startswith("naml"):
        b = eng._stage(eng._arrays(xs[:4], "his"), eng._arrays(xs[4:], "pred"), y)
        step = lambda: eng._train_kernels(b, C)
    else:
        b, expand = eng._stage(eng._uidx(xs[0]), xs[1], xs[2], y, False)
        step = lambda: eng._train_kernels(b, C, expand)
    n0 = count()
    step()
    n1 = count()
    eng.eval_loss(*xs, y)
    n2 = count()
    cat, (his_idx, cand_idx, cand_imp) = catalogue(kind)
    cache = eng.encode_catalogue(*cat)
    n3 = count()
    if kind.startswith("lstur"):
        eng.user_vectors_cached(cache, xs[0], his_idx)
    elif kind == "npa":
        eng.user_state_cached(cache, xs[0], his_idx)
    else:
        eng.score_cached(cache, his_idx, cand_idx, cand_imp, return_user=True)
    n4 = count()
    torch.cuda.synchronize()
    eng.check_oob()
    return n1 - n0, n2 - n1, n4 - n3


@pytest.mark.parametrize("kind", KINDS)
def test_launch_counts(hip, kind):
    got = launch_counts(kind)
    print(f"{kind}: train step {got[0]}, eval_loss {got[1]}, cached user vectors {got[2]} launches")
    assert got == EXPECTED[kind]
