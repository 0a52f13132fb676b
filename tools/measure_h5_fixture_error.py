"""Largest error of the eleven fixture tests of tests/test_gradients_gpu.py as a fraction of the tolerance rtol 2e-4 / atol 2e-5 they had
before it was tightened: prints one TOLFRAC line per fixture and output (the block at the top of profiles/r09_h5_error.txt).

    python tools/measure_h5_fixture_error.py
"""
import json, pathlib, sys
import numpy as np, torch
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from vod_amd.gradients import RetrievalGradients
G = ROOT / "tests" / "golden"
man = json.loads((G / "manifest.json").read_text())
RT, AT = 2e-4, 2e-5
names = ["retrieval_grad_2d", "retrieval_grad_3d", "retrieval_grad_nopos", "retrieval_grad_padded", "retrieval_grad_inbatch",
         "retrieval_aux_guidance_sparse", "retrieval_aux_guidance_zero", "retrieval_aux_self_supervision", "retrieval_aux_score_decay",
         "retrieval_aux_all", "retrieval_aux_all_nopos"]
worst = 0.0
for name in names:
    g = np.load(G / f"{name}.npz")
    cfg = man[name]["params"].get("config", {})
    qt = torch.tensor(g["q"], device="cuda", requires_grad=True); st = torch.tensor(g["s"], device="cuda", requires_grad=True)
    batch = {f"section__{k}": torch.tensor(g[k], device="cuda") for k in ("score", "relevance", "sparse", "dense")}
    out = RetrievalGradients(**cfg)(batch=batch, query_encoding=qt, section_encoding=st)
    out.loss.backward()
    pairs = {"loss": (out.loss, g["loss"]), "dq": (qt.grad, g["dq"]), "ds": (st.grad, g["ds"])}
    for k, v in out.diagnostics.items():
        pairs[k] = (v, g[f"diag_{k}"] if f"diag_{k}" in g.files else g[k])
    for k, (got, want) in pairs.items():
        got = got.detach().double().cpu().numpy(); want = np.asarray(want, dtype=np.float64)
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        if not fin.any():
            print(f"TOLFRAC {name} {k} all-NaN"); continue
        err = np.abs(got - want)[fin]
        frac = float(np.max(err / (AT + RT * np.abs(want[fin]))))
        worst = max(worst, frac)
        print(f"TOLFRAC {name} {k} max_abs_err={err.max():.3e} max|want|={np.abs(want[fin]).max():.3e} fraction_of_TOL={frac:.5f}")
print(f"TOLFRAC worst fraction_of_TOL={worst:.5f}")
