"""The example training scripts of this repository, run as a user runs them (`python examples/<script>.py ...`, here in-process
through runpy with the command line set): examples/bpr_synthetic.py and examples/dlrm_synthetic.py write the training / evaluation
loops of the TF-2 examples (tape-style `train_step` under `@tf.function`, keras metrics, evaluation lines) against this package,
on synthetic data with a planted preference model, so training must visibly move the validation AUC."""
import os
import re
import runpy
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_example(name, args, capsys, monkeypatch):
    """runs examples/<name> as __main__ with `args` on its command line; returns its printed lines"""
    path = os.path.join(ROOT, "examples", name)
    monkeypatch.setattr(sys, "argv", [path] + list(args))
    capsys.readouterr()
    runpy.run_path(path, run_name="__main__")
    return [l for l in capsys.readouterr().out.splitlines() if l.strip()]


def test_bpr_citeulike_script_runs_unmodified(capsys, monkeypatch):
    lines = _run_example("bpr_synthetic.py", ["--iters", "1000", "--eval-interval", "1000"], capsys, monkeypatch)
    lines = [l for l in lines if l.startswith("Iter:")]
    assert len(lines) == 2, lines                                        # evaluations at iteration 0 and 1000
    it, loss, auc = zip(*[(int(m.group(1)), float(m.group(2)), float(m.group(3)))
                          for m in (re.match(r"Iter: (\d+), Loss: ([-\d.]+), AUC: ([\d.]+)", l) for l in lines)])
    assert it == (0, 1000)
    assert abs(auc[0] - 0.5) < 0.03                                      # uniform(-0.05, 0.05) tables rank at random
    assert auc[1] > auc[0] + 0.05, lines                                 # 1000 Adam steps of batch 1000 later it does not
    assert 0.0 < loss[1] < 100.0                                        # (keras Mean over the tuple (loss, l2_loss))
    assert "Recall(50, 100)" in lines[1]


def test_dlrm_criteo_script_runs_unmodified(capsys, monkeypatch):
    lines = _run_example("dlrm_synthetic.py", ["--iters", "300"], capsys, monkeypatch)
    vals = [re.match(r"iter (\d+): train loss ([-\d.]+)\s+validation AUC ([\d.]+)", l) for l in lines]
    assert len(vals) == 3 and all(vals), lines
    assert [int(m.group(1)) for m in vals] == [100, 200, 300]
    loss = [float(m.group(2)) for m in vals]
    auc = [float(m.group(3)) for m in vals]
    # the planted model's dense and categorical parts are learnable: the training loss falls and the validation AUC leaves 0.5
    assert loss[-1] < loss[0], lines
    assert auc[-1] > 0.5 + 0.05, lines
