#!/usr/bin/env python3
"""The bits of the four state encoders.  The recurrent two (csrc/lstm.hip, csrc/gru.hip over csrc/seq_chain.h and csrc/seq_bwd.h): one SHA-256 per
output tensor of `lstm_encode_train` / `gru_encode_train` and of their backward, for seeded stores at the shapes the GPU tests
use -- (E, H) = (8, 16), (40, 96), (128, 256) at U = 17 with T = 1 and T = 37 (a partly filled second tile; one step, and a chunk
boundary), and U = 1, 5, 16, 25 at (40, 96) with T = 37 -- for both cells, both variants (`set_lstm_variant`), with and without an
initial state.  Per case: h, h_T, (c_T), every weight gradient, d_h0 (d_c0) when there
is an initial state, and d_table (`train_table=True`).  The loss weights every output with seeded noise, so g_h, g_hT and g_cT all
arrive.
The attention encoder and the transformer encoder (csrc/attn.hip, csrc/block.hip over csrc/attn_dev.h): h, every parameter gradient
and d_table of `attn_encode_train` / `transformer_encode_train` with `train_table=True` under the same kind of loss, at shapes that
cross every edge of the kernels the two share with each other and with the recurrent pair -- attention at (E, H, heads) = (8, 16, 1),
(40, 96, 3), (128, 256, 4) with (U, T) = (1, 1), (5, 63), (9, 130) (U T = 1170 > 1024: two weight-gradient segments; T = 130: three
64-row tiles), window None and 5, ALiBi off and on; the transformer with two layers at (E, H, heads, F) = (8, 16, 1, 48) (a
half-filled feed-forward chunk) and (40, 96, 3, 272) (F and 3H above 256: the K-blocked walk of the dense linear), relu and gelu,
(U, T) = (5, 63), (9, 130).

A refactor of these kernels that reorders no sum leaves every digest as it is: run this once per library (`RECNN_HIP_LIB` selects
one), in separate processes, and compare the "digests" of the two outputs -- or compare against profiles/seq_bits.json, which holds
them for the toolchain and GPU named in it.  Prints one JSON line.
usage: python tools/seq_bits.py [--out profiles/seq_bits.json] [--against OTHER.json]   (exit status 1 if a digest differs)"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

# (E, H, U, T)
CASES = [(E, H, 17, T) for E, H in ((8, 16), (40, 96), (128, 256)) for T in (1, 37)] + [(40, 96, U, 37) for U in (1, 5, 16, 25)]
N_ITEMS = 97


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def seeded(E, H, U, T, dev):
    """(store, randn, table, gen) of a case: histories of T + 2 .. T + 8 elements, a table that requires grad."""
    from recnn_amd.data.store import ReplayStore
    rng = np.random.default_rng(1000 * H + 10 * U + T)
    lens = rng.integers(T + 2, T + 9, size=U)
    off = np.zeros(U + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    items = rng.integers(0, N_ITEMS, size=int(off[-1])).astype(np.int32)
    ratings = (rng.integers(1, 11, size=int(off[-1])) * 0.5 - 2.5).astype(np.float32)
    store = ReplayStore.from_arrays(items, ratings, off, dev)
    gen = torch.Generator().manual_seed(7 * H + U + T)
    randn = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    return store, randn, randn(N_ITEMS, E).requires_grad_(True), gen


def case(cell, E, H, U, T, with_state, dev):
    from recnn_amd.nn import functional as F
    store, randn, table, gen = seeded(E, H, U, T, dev)
    nstate = 2 if cell == "lstm" else 1
    module = (torch.nn.LSTM if cell == "lstm" else torch.nn.GRU)(E + 1, H, batch_first=True)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(0.3 * torch.randn(p.shape, generator=gen))
    module = module.to(dev)
    states = [randn(U, H).requires_grad_(True) for _ in range(nstate)] if with_state else None
    init = None if states is None else (tuple(states) if cell == "lstm" else states[0])
    encode_train = F.lstm_encode_train if cell == "lstm" else F.gru_encode_train
    h, last = encode_train(module, store, table, np.arange(U, dtype=np.int32), T, init, t0=1, train_table=True)
    last = last if cell == "lstm" else (last,)
    outs = dict(zip(("h", "h_T", "c_T"), (h, *last)))
    loss = sum((o * randn(*o.shape)).sum() for o in outs.values())
    loss.backward()
    d = {k: sha(v) for k, v in outs.items()}
    for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
        d["d_" + n] = sha(getattr(module, n).grad)
    for n, s in zip(("d_h0", "d_c0"), states or ()):
        d[n] = sha(s.grad)
    d["d_table"] = sha(table.grad)
    return d


# attention: (E, H, heads) x (U, T) x window x alibi; transformer (two layers): (E, H, heads, F) x activation x (U, T)
ATTN_CASES = [(E, H, heads, U, T, window, alibi) for E, H, heads in ((8, 16, 1), (40, 96, 3), (128, 256, 4))
              for U, T in ((1, 1), (5, 63), (9, 130)) for window in (None, 5) for alibi in (False, True)]
BLOCK_CASES = [(E, H, heads, ffn, act, U, T) for E, H, heads, ffn in ((8, 16, 1, 48), (40, 96, 3, 272)) for act in ("relu", "gelu")
               for U, T in ((5, 63), (9, 130))]


def module_case(enc, encode_train, E, H, U, T, dev):
    """h, every parameter gradient and d_table of one attention / transformer encoder under the seeded-noise loss."""
    store, randn, table, gen = seeded(E, H, U, T, dev)
    with torch.no_grad():
        for p in enc.parameters():
            p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    enc = enc.to(dev)
    h = encode_train(enc, store, table, np.arange(U, dtype=np.int32), T, t0=1, train_table=True)
    (h * randn(*h.shape)).sum().backward()
    d = {"h": sha(h), "d_table": sha(table.grad)}
    d.update(("d_" + n, sha(p.grad)) for n, p in enc.named_parameters())
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--against", default=None, help="an earlier output: report every digest that differs")
    a = ap.parse_args()
    from recnn_amd.nn import functional as F
    dev = torch.device("cuda")
    digests = {}
    for cell in ("lstm", "gru"):
        for variant in ("fused", "chunked"):
            F.set_lstm_variant(variant)
            for E, H, U, T in CASES:
                for with_state in (False, True):
                    key = f"{cell} {variant} E={E} H={H} U={U} T={T} state={int(with_state)}"
                    digests[key] = case(cell, E, H, U, T, with_state, dev)
    F.set_lstm_variant("chunked")
    from recnn_amd.nn import AttentionEncoder, TransformerStateEncoder
    for E, H, heads, U, T, window, alibi in ATTN_CASES:
        enc = AttentionEncoder(E + 1, H, heads, window=window, alibi=alibi)
        digests[f"attn E={E} H={H} heads={heads} U={U} T={T} window={window} alibi={int(alibi)}"] = \
            module_case(enc, F.attn_encode_train, E, H, U, T, dev)
    for E, H, heads, ffn, act, U, T in BLOCK_CASES:
        enc = TransformerStateEncoder(E + 1, H, heads, num_layers=2, dim_feedforward=ffn, activation=act)
        digests[f"transformer E={E} H={H} heads={heads} F={ffn} act={act} U={U} T={T}"] = \
            module_case(enc, F.transformer_encode_train, E, H, U, T, dev)
    res = {"tool": "seq_bits", "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "torch": torch.__version__, "hip": torch.version.hip, "lib": os.environ.get("RECNN_HIP_LIB", "in-tree"),
           "cases": len(digests), "digests": digests}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            head = {k: v for k, v in res.items() if k != "digests"}           # one line per case: the file is read in diffs
            f.write(json.dumps(head)[:-1] + ', "digests": {\n'
                    + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in digests.items()) + "\n}}\n")
    print(json.dumps(res))
    if a.against:
        other = json.load(open(a.against))["digests"]
        bad = [(k, t) for k in sorted(set(other) | set(digests)) for t in sorted(set(other.get(k, {})) | set(digests.get(k, {})))
               if other.get(k, {}).get(t) != digests.get(k, {}).get(t)]
        for k, t in bad:
            print(f"DIFFERENT {k}: {t}", file=sys.stderr)
        print(f"{sum(len(v) for v in digests.values())} digests, {len(bad)} differ from {a.against}", file=sys.stderr)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
