"""eda_amd.inference on the host: the counters of DeviceGroundingEvaluator against the goldens the REFERENCE's evaluator
produced (tests/golden/eval_counts.npz, the file tests/test_evaluator.py uses), and the torch form of decode_grounding
against an fp64 form (tests/inference_fixtures.py), tie rule included.  The GPU tests compare the kernel with both."""
import os

import numpy as np
import torch

import eval_fixtures as EF
import inference_fixtures as IF

GOLD = os.path.join(os.path.dirname(__file__), "golden", "eval_counts.npz")


def check_golden_counters(dev, how="all"):
    from eda_amd.inference import DeviceGroundingEvaluator
    g = np.load(GOLD)
    for case, (seed, only_root, filt) in EF.CASES.items():
        ep = IF.to_device(EF.make_end_points(seed), dev)
        ev = DeviceGroundingEvaluator(only_root=only_root, thresholds=[0.25, 0.5], topks=[1, 5, 10], prefixes=EF.PREFIXES,
                                      filter_non_gt_boxes=filt)
        for _ in range(2):
            if how == "all":
                ev.evaluate_all(ep)
            else:
                for p in EF.PREFIXES:
                    ev.evaluate(ep, p)
        keys = EF.counter_keys(ev)
        assert len(keys) == len(g[case + "_dets"])
        d, t = ev.dets, ev.gts
        dets = np.array([float(d[k]) for k in keys])
        gts = np.array([float(t[k]) for k in keys])
        bad = [(k, x, e) for k, x, e in zip(keys, dets, g[case + "_dets"]) if x != e]
        assert not bad, (case, bad[:5])
        np.testing.assert_allclose(gts, g[case + "_gts"], rtol=0, atol=1e-12, err_msg=case)
        assert dets.sum() > 0 and (dets < gts - 0.5).any()


def test_device_evaluator_counters_equal_the_reference_cpu():
    check_golden_counters("cpu")


def test_single_prefix_evaluate_is_a_drop_in_cpu():
    check_golden_counters("cpu", how="each")


def test_decode_torch_form_against_fp64():
    from eda_amd.inference import decode_grounding
    total = left = 0
    for case, ep, prefixes, only_root, filt in IF.fixture_cases():
        out = decode_grounding(ep, prefixes=prefixes, topk=10, targets=ep, filter_non_gt_boxes=filt, only_root=only_root)
        G = 1 if only_root else ep["positive_map"].shape[1]
        assert out["top_query"].shape == (len(prefixes), 2, 8, G, 10) and out["top_query"].dtype == torch.int32
        assert out["top_corners"].shape == out["top_box"].shape == (len(prefixes), 2, 8, G, 10, 6)
        n, lo, err = IF.compare_with_fp64(out, ep, prefixes, only_root, filt)
        print(f"{case}: {n} slots, {lo} near-ties left out, largest score error {err:.3e}")
        total, left = total + n, left + lo
        half = 0.5 * out["top_box"][..., 3:].clamp(min=1e-6)
        assert torch.equal(out["top_corners"], torch.cat([out["top_box"][..., :3] - half, out["top_box"][..., :3] + half], -1))
    assert left <= IF.MAX_LEFT_OUT * total


def _tie_case():
    """Queries 3, 7, 11 and 20 have EXACTLY the same token scores and the highest score for object 0; the rest fall off."""
    ep = EF.make_end_points(21)
    for p in EF.PREFIXES:
        ep[f"{p}sem_cls_scores"].zero_()
        tok = (ep["positive_map"][:, 0] > 0).float()                        # (B, T)
        ep[f"{p}sem_cls_scores"][:, :, :] = -0.01 * torch.arange(48.0)[None, :, None] * tok[:, None, :]
        for q in (20, 11, 7, 3):
            ep[f"{p}sem_cls_scores"][:, q] = 3.0 * tok
            ep[f"{p}proj_queries"][:, q] = ep[f"{p}proj_queries"][:, 3]
    for k in IF.AUX:
        ep[k].zero_()
    return ep


def check_tie_rule(dev):
    from eda_amd.inference import decode_grounding
    ep = IF.to_device(_tie_case(), dev)
    out = decode_grounding(ep, prefixes=EF.PREFIXES, topk=10, targets=ep, only_root=True)
    q = out["top_query"].cpu()
    s = out["top_score"].cpu()
    # position alignment: the four equal queries lead, lowest index first, with exactly equal scores
    assert q[:, 0, :, 0, :4].tolist() == [[[3, 7, 11, 20]] * 8] * len(EF.PREFIXES)
    assert bool((s[:, 0, :, 0, :4] == s[:, 0, :, 0, :1]).all())
    # ... then the others by descending score, which here is ascending query index
    assert q[:, 0, :, 0, 4:].tolist() == [[[0, 1, 2, 4, 5, 6]] * 8] * len(EF.PREFIXES)
    # semantic alignment: the four identical projected queries are adjacent in the ranking, lowest index first
    for pi in range(len(EF.PREFIXES)):
        for b in range(8):
            row = q[pi, 1, b, 0].tolist()
            if 3 in row[:7]:
                i = row.index(3)
                assert row[i:i + 4] == [3, 7, 11, 20], row


def test_tie_rule_lowest_query_first_cpu():
    check_tie_rule("cpu")


def test_decode_without_targets_and_single_alignment():
    from eda_amd.inference import decode_grounding
    ep = EF.make_end_points(21)
    both = decode_grounding(ep, prefixes=["last_"], targets=ep)
    sem = decode_grounding(ep, prefixes=["last_"], alignment="semantic", topk=5)
    assert "top_iou" not in sem and sem["top_query"].shape == (1, 1, 8, 132, 5)
    # without targets the auxiliary maps are not read: same ranking only where they are zero; shapes and boxes are checked
    assert torch.equal(decode_grounding(ep, prefixes=["last_"], alignment="semantic", topk=5, targets=ep)["top_query"],
                       both["top_query"][:, 1:, ..., :5])


def test_counters_api():
    from eda_amd.inference import DeviceGroundingEvaluator
    ev = DeviceGroundingEvaluator(prefixes=["last_"])
    ep = EF.make_end_points(21)
    ev.evaluate_all(ep)
    ev.print_stats()
    assert ev.gts[("last_", 0.25, 1, "bbf")] == 8
    assert sum(ev.gts[k] for k in ("vd", "vid")) == 8 + 2e-14
    ev.synchronize_between_processes()          # no process group: totals are kept
    assert ev.gts[("last_", 0.25, 1, "bbf")] == 8
    ev.reset()
    assert ev.dets[("last_", 0.25, 1, "bbf")] == 0 and ev.gts["vd"] == 1e-14


def test_library_declares_the_decode_entry_points():
    import re
    from eda_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "eda_hip.h")).read()
    for name in ("eda_ground_decode_f32", "eda_ground_decode_supported", "eda_ground_decode_lds_bytes"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header)
    # the prototype and the ctypes row have the same number of parameters
    proto = re.search(r"int eda_ground_decode_f32\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["eda_ground_decode_f32"][1])
