"""The stop rule of the power iterations (diffusion_pullback_amd/pullback.py) on the CPU, driven through a stub engine that returns a scripted conv.

dpb_orth answers a NaN or an inf in W = J^T J V or in V_prev with conv = (NaN, NaN) and a NaN basis (include/dpb.h).  The loops that read conv --
_pullback, local_encoder_pullback_batch and the decoder loop -- must then raise DpbError naming the iteration (and, in the batch form, the samples),
and never count such an iteration as converged: before the rule conv[1] came back 0 beside a NaN basis (a NaN-dropping maximum), `0 <= thr` held, and
the loop returned NaN as a converged result.  The stub scripts exactly that shape as well.  A finite script must stop where it always did."""
import types

import pytest
import torch

from diffusion_pullback_amd import lib as L
from diffusion_pullback_amd.pullback import PullbackUNet

NAN = float("nan")
N_IN, N_H, K = 12, 6, 2


class _StubEngine:
    """what the three loops touch of an Engine, on CPU tensors; orth / iterate return the next entry of the conv script"""
    n_in, max_batch = N_IN, 4
    tape = types.SimpleNamespace(taps={"o": 0, "eps": 1})

    def __init__(self, script):
        self.script, self.calls = script, 0

    def primal(self, x, t, ctx, key):
        self.batch = x.shape[0]

    def tap_numel(self, key):
        return N_H

    def jvp(self, key, V):
        return torch.zeros(V.shape[0], N_H)

    def vjp(self, key, U):
        return torch.zeros(U.shape[0], N_IN)

    def jvp_between(self, src, dst, V):
        return torch.zeros(V.shape[0], N_IN)

    def vjp_between(self, src, dst, U):
        return torch.zeros(U.shape[0], N_H)

    def _next(self):
        c = self.script[min(self.calls, len(self.script) - 1)]
        self.calls += 1
        return torch.tensor(c, dtype=torch.float32)

    def orth(self, W, Vprev):
        return Vprev.clone(), torch.ones(len(W)), self._next()

    def iterate(self, key, V, n_iters):
        return V, torch.zeros(V.shape[0], N_H), torch.ones(V.shape[0]), self._next()


def _net(script):
    eng = _StubEngine(script)
    return types.SimpleNamespace(engine=eng, max_rank=8, device="cpu", verbose=False, k_shard_group=False, _tap=lambda op, block_idx: "o",
                                 _decoder_tap=lambda op, block_idx: "o")


def _single(script, **kw):
    net = _net(script)
    V0 = torch.eye(K, N_IN)
    args = dict(min_iter=1, max_iter=10, thr=1e-3)
    args.update(kw)
    out = PullbackUNet._pullback(net, torch.zeros(1, N_IN), 1.0, None, None, None, K, 1, args["min_iter"], args["max_iter"], args["thr"], V0)
    return net, out


FINITE = [[1.0, 0.5], [0.5, 0.2], [0.1, 0.05]]


@pytest.mark.parametrize("bad", [[NAN, NAN], [NAN, 0.0], [0.0, NAN], [float("inf"), 1.0]], ids=["nan-nan", "nan-0", "0-nan", "inf"])
def test_pullback_raises_at_the_first_non_finite_conv(bad):
    """finite conv for iterations 0 .. 2, then non-finite from iteration 3 on: DpbError at iteration 3, after exactly four re-orthonormalisations.
    (NaN, 0) is what the kernels returned before conv[1] propagated NaN: `0 <= thr` must not pass for a converged result"""
    net = _net(FINITE + [bad])
    with pytest.raises(L.DpbError, match=r"iteration 3 are not finite") as err:
        PullbackUNet._pullback(net, torch.zeros(1, N_IN), 1.0, None, None, None, K, 1, 1, 10, 1e-3, torch.eye(K, N_IN))
    assert "sample" not in str(err.value)
    assert net.engine.calls == 4 and len(net.last_history) == 4


def test_pullback_does_not_raise_on_small_finite_conv_before_min_iter():
    """a converged figure before min_iter neither stops nor raises; the first one after it stops"""
    net, _ = _single([[1.0, 0.0]] * 3 + [[1.0, 1.0]] * 2 + [[1e-6, 1e-6]], min_iter=3)
    assert net.last_iters == 6 and net.engine.calls == 6


def test_pullback_clean_script_stops_where_it_always_did():
    """viol <= thr and i > min_iter: with min_iter = 1 the first iteration that may stop is i = 2"""
    net, (u, s, vT) = _single([[1.0, 1.0], [1.0, 1e-9], [1.0, 1.0], [0.5, 5e-4], [0.1, 1e-9]])
    assert net.last_iters == 4 and net.engine.calls == 4 and net.last_dist == 0.5
    assert tuple(u.shape) == (N_H, K) and tuple(s.shape) == (K,) and tuple(vT.shape) == (K, N_IN)
    net, _ = _single([[1.0, 1.0]], max_iter=7)
    assert net.last_iters == 7                                     # never converged: max_iter iterations, as before


def test_decoder_loop_raises_the_same_way():
    net = _net(FINITE + [[NAN, NAN]])
    with pytest.raises(L.DpbError, match=r"iteration 3 are not finite"):
        PullbackUNet._decoder_pullback(net, torch.zeros(1, N_IN), 1.0, None, None, None, K, 1, 1, 10, 1e-3, torch.eye(K, N_H))
    net = _net(FINITE + [[NAN, NAN]])
    with pytest.raises(L.DpbError, match=r"iteration 3 are not finite"):             # thr = None (no early stop) reads conv all the same
        PullbackUNet._decoder_pullback(net, torch.zeros(1, N_IN), 1.0, None, None, None, K, 1, 1, 10, None, torch.eye(K, N_H))
    net = _net([[1.0, 1.0], [1.0, 1.0], [0.5, 1e-4]])
    PullbackUNet._decoder_pullback(net, torch.zeros(1, N_IN), 1.0, None, None, None, K, 1, 1, 10, 1e-3, torch.eye(K, N_H))
    assert net.last_iters == 3


def _batch(script, B=3, **kw):
    net = _net(script)
    args = dict(pca_rank=K, min_iter=1, max_iter=10, convergence_threshold=1e-3, V0=torch.eye(K, N_IN))
    args.update(kw)
    return net, PullbackUNet.local_encoder_pullback_batch(net, torch.zeros(B, N_IN), 1.0, None, None, None, **args)


def test_batch_form_names_the_iteration_and_the_samples():
    fin = [[1.0, 0.5]] * 3
    net = _net([fin, fin, fin, [[NAN, NAN], [0.5, 0.5], [NAN, 0.0]]])
    with pytest.raises(L.DpbError, match=r"iteration 3 are not finite for sample\(s\) \[0, 2\] of the batch"):
        PullbackUNet.local_encoder_pullback_batch(net, torch.zeros(3, N_IN), 1.0, None, None, None, pca_rank=K, min_iter=1, max_iter=10,
                                                  convergence_threshold=1e-3, V0=torch.eye(K, N_IN))
    assert net.engine.calls == 4
    net = _net([fin, fin, fin, [[0.5, 0.5], [float("-inf"), NAN], [0.5, 0.5]]])
    with pytest.raises(L.DpbError, match=r"iteration 3 are not finite for sample\(s\) \[1\] of the batch"):
        PullbackUNet.local_encoder_pullback_batch(net, torch.zeros(3, N_IN), 1.0, None, None, None, pca_rank=K, min_iter=1, max_iter=10,
                                                  convergence_threshold=1e-3, V0=torch.eye(K, N_IN))


def test_batch_form_clean_script_stops_where_it_always_did():
    """sample 0 meets the rule at i = 2, sample 1 at i = 4, sample 2 never: iters = (3, 5, max_iter), and the loop runs max_iter iterations"""
    big, ok = [1.0, 1.0], [0.1, 1e-6]
    script = [[ok, big, big], [ok, big, big], [ok, big, big], [big, big, big], [big, ok, big], [big, big, big]]
    net, (u, s, vT, iters) = _batch(script, max_iter=8)
    assert iters.tolist() == [3, 5, 8] and net.last_iters == 8 and net.engine.calls == 8
    assert tuple(u.shape) == (3, N_H, K) and tuple(s.shape) == (3, K) and tuple(vT.shape) == (3, K, N_IN)
    net, (_, _, _, iters) = _batch([[ok, ok, ok]], max_iter=8)
    assert iters.tolist() == [3, 3, 3] and net.engine.calls == 3   # all stop at the first i > min_iter: the loop ends there
