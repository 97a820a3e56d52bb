"""Train-time scene augmentation and box targets on the GPU (csrc/augment.hip through eda_amd/augment.py): bit
equality with the CPU form at 8 x 50 000 points (explicit draws and Philox draws), the reference's golden cases, the
device counter across captured replays, and the stage inside the pipelined training step."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import augment_fixtures as F
from eda_amd import augment as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_bank(dev, n_scans, n_points, seed=0, n_objects=(40, 90), xyz_from=None):
    """Synthetic scans: points in a room (or the given coordinates), ~90 % of them in disjoint objects, detector boxes."""
    rng = np.random.RandomState(seed)
    bank = A.SceneBank(dev, capacity=2)
    for s in range(n_scans):
        xyz = rng.uniform([-3, -2.5, 0], [3, 2.5, 3], (n_points, 3)) if xyz_from is None else xyz_from[s]
        col = rng.rand(n_points, 3).astype(np.float32)
        k = rng.randint(*n_objects) if s != 1 else 300          # one scan with more than 132 objects
        owner = np.where(rng.rand(n_points) < 0.9, rng.randint(0, k, n_points), -1)
        objs = [np.flatnonzero(owner == i) for i in range(k)]
        c = rng.uniform(-2, 2, (30, 3))
        sz = rng.uniform(0.1, 1.0, (30, 3))
        bank.add_scan(xyz, col, objs, detected_boxes=np.concatenate([c - sz / 2, c + sz / 2], 1),
                      detected_class_ids=rng.randint(0, 485, 30))
    return bank


def batch_inputs(bank, rng, B, slots=None):
    slots = rng.choice(bank.n_slots, B, replace=False) if slots is None else np.asarray(slots)
    targets, keep = [], np.zeros((B, 132), bool)
    for b, s in enumerate(slots):
        n = bank.n_objects(int(s))
        targets.append(rng.choice(n, rng.randint(1, min(n, 20)), replace=False))
        keep[b] = rng.rand(132) < 0.8
    if 1 in slots:                                             # a target index >= 132
        targets[list(slots).index(1)][0] = 250
    return slots, targets, keep


def _equal(got, want, what=""):
    for k in F.KEYS:
        g = got[k].cpu()
        w = torch.as_tensor(want[k]) if not torch.is_tensor(want[k]) else want[k].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        assert torch.equal(g, w), (what, k, (g != w).sum().item())


@pytest.mark.parametrize("mode,augment_det,train", [("butd", True, True), ("none", False, True),
                                                    ("butd_cls", False, True), ("butd", False, False)])
def test_kernel_equals_cpu_form_8x50k(mode, augment_det, train):
    dev = torch.device("cuda", 0)
    bank = make_bank(dev, 10, 50000)
    rng = np.random.RandomState(1)
    B = 8
    slots, targets, keep = batch_inputs(bank, rng, B, slots=[0, 1, 2, 3, 4, 5, 6, 9])
    params = A.draw_params(rng, B, rotate=[True, False] * 4, augment_det=augment_det) if train else A.identity_params(B)
    dcls = rng.randint(0, 485, (B, 132)) if mode == "butd_cls" else None
    kw = dict(detected_mode=mode, augment_det=augment_det, train=train, det_class_ids=dcls)
    ints = A.pack_targets(bank, slots, targets, keep, dcls)
    # explicit draws
    u = np.random.RandomState(2).rand(B, 50000, 6)
    ex = {"noise": u[..., :3] * 5e-3, "color_factor": 0.98 + 0.04 * u[..., 3:]}
    got = A.augment_batch(bank, slots, params, targets, keep, explicit=ex, **kw)
    want = A.cpu_form(bank, ints, params, train=train, det_mode=A.DET_MODES[mode], augment_det=augment_det, explicit=ex)
    _equal(got, want, "explicit")
    # Philox draws at (seed, counter)
    got = A.augment_batch(bank, slots, params, targets, keep, seed=1234, counter=77, **kw)
    want = A.cpu_form(bank, ints, params, train=train, det_mode=A.DET_MODES[mode], augment_det=augment_det, seed=1234,
                      counter=77)
    _equal(got, want, "rng")
    for k, t in got.items():
        if t.dtype.is_floating_point:
            assert torch.isfinite(t).all(), k             # (outputs come from the NaN-poisoned allocator)
    if train:
        assert (got["point_instance_label"][1] >= 0).any()


@pytest.mark.parametrize("name", F.CASES)
def test_golden_cases_on_gpu(name):
    g = F.load(name)
    bank = A.SceneBank("cuda")
    slot = F.add_to_bank(bank, g)
    p, explicit, kw = F.inputs(g)
    out = A.augment_batch(bank, [slot], p[None], explicit=explicit, **kw)
    for k in F.KEYS:
        got, want = out[k].cpu().numpy()[0], g[k]
        if want.dtype.kind == "f" and k != "box_label_mask":
            assert F.ulps_f32(got, want).max() <= 1, k
        else:
            np.testing.assert_array_equal(got, want, err_msg=k)


def test_draws_statistics_and_keys():
    dev = torch.device("cuda", 0)
    n = 50000
    bank = A.SceneBank(dev)
    bank.add_scan(np.zeros((n, 3)), np.full((n, 3), 0.5, np.float32), [np.arange(100)])
    p = A.identity_params(4)                      # train with identity geometry: the points are the noise itself
    slots, targets = [0, 0, 0, 0], [[0]] * 4
    a = A.augment_batch(bank, slots, p, targets, seed=9, counter=5)
    b = A.augment_batch(bank, slots, p, targets, seed=9, counter=5)
    c = A.augment_batch(bank, slots, p, targets, seed=9, counter=6)
    d = A.augment_batch(bank, slots, p, targets, seed=10, counter=5)
    _equal(a, b, "same key")
    pc = a["point_clouds"].double()
    assert not torch.equal(pc, c["point_clouds"].double()) and not torch.equal(pc, d["point_clouds"].double())
    assert not torch.equal(pc[0], pc[1])           # another scene position draws other values for the same scan
    noise = pc[..., :3]
    assert noise.min() >= 0 and noise.max() < 5e-3 + 1e-9
    assert abs(noise.mean().item() - 2.5e-3) < 2e-5
    m = torch.tensor(A.MEAN_RGB, device=dev)
    f = (pc[..., 3:] + m) / 0.5
    assert f.min() >= 0.98 - 1e-6 and f.max() < 1.02 + 1e-6
    assert abs(f.mean().item() - 1.0) < 1e-3


def test_stage_replays_advance_counter():
    dev = torch.device("cuda", 0)
    bank = make_bank(dev, 6, 20000, seed=3)
    rng = np.random.RandomState(4)
    slots, targets, keep = batch_inputs(bank, rng, 4)
    params = A.draw_params(rng, 4, augment_det=True)
    stage = A.AugmentStage(bank, 4, detected_mode="butd", augment_det=True, seed=42, counter=1000)
    stage.set_inputs(slots, params, targets, keep)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        stage()
    torch.cuda.synchronize()
    assert stage.get_counter() == 1000                 # capturing runs nothing
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        want = A.augment_batch(bank, slots, params, targets, keep, detected_mode="butd", augment_det=True, seed=42,
                               counter=1000 + i)
        _equal(stage.out, want, f"replay {i}")
        for k, t in stage.out.items():
            if t.dtype.is_floating_point:
                assert torch.isfinite(t).all(), k
    assert stage.get_counter() == 1003
    stage.set_counter(1001)
    g.replay()
    torch.cuda.synchronize()
    _equal(stage.out, A.augment_batch(bank, slots, params, targets, keep, detected_mode="butd", augment_det=True,
                                      seed=42, counter=1001), "after set_counter")


def test_pipelined_step_with_augment_stage():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    import check_graph_vs_eager as C
    from eda_amd import pipeline
    from eda_amd.parallel import FlatParams
    from eda_amd import synthetic
    dev = torch.device("cuda", 0)
    scenes, points, tokens, steps = 2, 20000, 24, 5
    xyz = [synthetic.batch([s], points)[0, :, :3].astype(np.float64) for s in range(6)]
    bank = make_bank(dev, 6, points, seed=5, xyz_from=xyz)
    rng = np.random.RandomState(6)
    seq = []
    for i in range(steps + 1):
        slots, targets, keep = batch_inputs(bank, rng, scenes, slots=[(2 * i) % 6, (2 * i + 1) % 6])
        seq.append((slots, targets, keep, A.draw_params(rng, scenes)))
    seed, c0 = 77, 500
    stage = A.AugmentStage(bank, scenes, seed=seed, counter=c0)
    base = bench.make_inputs(0, scenes, dev, points, tokens)
    produced = set(stage.produces)

    def eager_batch(i):
        s, t, k, p = seq[i]
        aug = A.augment_batch(bank, s, p, t, k, seed=seed, counter=c0 + i)
        return dict(base, **aug)

    def fed(i):
        s, t, k, p = seq[i]
        packed = {kk: v.to(dev) for kk, v in stage.pack(s, p, t, k).items()}
        return dict({kk: v for kk, v in base.items() if kk not in produced}, **packed)

    eager_batches = [eager_batch(i) for i in range(steps + 1)]
    assert eager_batches[0]["point_clouds"].shape == base["point_clouds"].shape
    a = C.make(0, dev, num_queries=64, num_decoder_layers=2)
    b = copy.deepcopy(a)

    def trainer(model):
        flat = FlatParams(model)

        def backward(loss):
            with flat.deferred_wgrad():
                loss.backward()
            flat.collect_grads()

        def update():
            flat.clip_grad_norm_(0.1)
            with torch.no_grad():
                for gp in flat.groups.values():
                    gp.add_(gp.grad, alpha=-0.05)
        return backward, update

    loss_fn = lambda ep, batch: bench.synthetic_loss(ep)          # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        backward, update = trainer(a)
        eager = []
        for i in range(steps):
            loss = loss_fn(a(eager_batches[i]), eager_batches[i])
            backward(loss)
            update()
            eager.append(float(loss.detach()))
        torch.cuda.synchronize()
        backward, update = trainer(b)
        first = dict(eager_batches[0], **fed(0))
        pipe = pipeline.PipelinedTrainStep(b, first, loss_fn, backward, update, stream=side, pre_stage=stage)
        got = []
        for i in range(steps):
            loss = pipe.step(next_batch=fed(i + 1))
            torch.cuda.synchronize()
            got.append(float(loss.detach()))
            s, t, k, p = seq[i]
            ints = A.pack_targets(bank, s, t, k)
            want = A.cpu_form(bank, ints, p, seed=seed, counter=c0 + i)
            assert torch.equal(pipe.cur["point_clouds"].cpu(), torch.from_numpy(want["point_clouds"])), f"step {i}"
            assert torch.equal(pipe.cur["point_instance_label"].cpu(), torch.from_numpy(want["point_instance_label"]))
        assert stage.get_counter() == c0 + steps + 1
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert abs(eager[0] - got[0]) <= 1e-5 * abs(eager[0]), (eager, got)
    bad = max(abs(x - y) / max(abs(x), 1e-9) for x, y in zip(eager, got))
    assert bad < 2e-2, (eager, got)
