"""N4 wire formats: pickle dict / SemanticKITTI .label writers against the reference's recipe
(np.argmax of the softmax, learning_map_inv lookup, uint16) -- bit-exact."""
import pickle

import numpy as np
import pytest
import torch


def _reference_recipe(logits):
    y = torch.softmax(logits, dim=1).numpy()                 # generate_output.py:94-95
    return np.argmax(y, axis=1)


def test_inverse_label_map_matches_reference_yaml():
    import json
    import os
    from occdepth_amd.output import KITTI_LEARNING_MAP_INV, get_inv_map
    # learning_map_inv of the reference's occdepth/data/semantic_kitti/semantic-kitti.yaml, classes 0 .. 19
    fixture = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "semantic_kitti_learning_map_inv.json")
    with open(fixture) as f:
        assert json.load(f)["learning_map_inv"] == list(KITTI_LEARNING_MAP_INV)
    assert get_inv_map().dtype == np.int32 and get_inv_map()[[0, 1, 9, 19]].tolist() == [0, 10, 40, 81]


@pytest.mark.gpu
def test_writers_bit_exact_vs_reference_recipe(tmp_path, hip_lib):
    from occdepth_amd import output
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(2, 20, 16, 12, 8, generator=g)
    logits[0, 3, 1, 1, 1] = logits[0, 7, 1, 1, 1] = 9.0       # a tie: the first maximum must win
    batch = {"sequence": ["08", "08"], "frame_id": ["000000", "000005"],
             "fov_mask_1": [torch.ones(2, 5, dtype=torch.bool)] * 2, "cam_k": [torch.eye(3)[None]] * 2,
             "T_velo_2_cam": [torch.eye(4)[None]] * 2, "target": torch.randint(0, 20, (2, 16, 12, 8)).to(torch.uint8)}
    want = _reference_recipe(logits)
    paths = output.write_outputs(logits.cuda(), batch, str(tmp_path / "out"), "kitti")
    for i, p in enumerate(paths):
        d = pickle.load(open(p, "rb"))
        assert set(d) == {"y_pred", "target", "fov_mask_1", "cam_k", "T_velo_2_cam"}
        assert d["y_pred"].dtype == np.uint16 and np.array_equal(d["y_pred"], want[i].astype(np.uint16))
        assert d["target"].dtype == np.uint16
    assert paths[1].endswith("08/000005.pkl")
    labels = output.write_kitti_submission(logits.cuda(), batch, str(tmp_path / "sub"))
    inv = output.get_inv_map()
    for i, p in enumerate(labels):
        got = np.fromfile(p, dtype=np.uint16)
        assert np.array_equal(got, inv[want[i].reshape(-1)].astype(np.uint16))
    assert labels[0].endswith("sequences/08/predictions/000000.label")
