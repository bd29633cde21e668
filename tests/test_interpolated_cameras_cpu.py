"""scene.interpolate_poses / scene.interpolated_cameras (the rule of src/scene/dataset_readers.py:160-193) on key
cameras at frames 3, 7, 8 and 15: gaps of one and of more than one, a first frame that is not 0.  The blend and the spline are
computed again here, independently of the code under test."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytest.importorskip("scipy")
from scipy.spatial.transform import Rotation, RotationSpline  # noqa: E402

from gaussianhaircut_amd import scene  # noqa: E402
from gaussianhaircut_amd.scene.cameras import Camera, interpolate_poses, interpolated_cameras  # noqa: E402
from gaussianhaircut_amd.utils.graphics_utils import getWorld2View2  # noqa: E402

FRAMES = [3, 7, 8, 15]


def _keys(tensor_fov=False, sizes=((36, 64), (36, 64), (40, 60), (36, 64))):
    g = np.random.default_rng(11)
    R = Rotation.from_rotvec(g.normal(size=(4, 3)) * 0.4).as_matrix()
    T = g.normal(size=(4, 3)) + np.array([0.0, 0.0, 4.0])
    fx, fy = 0.5 + 0.1 * g.random(4), 0.8 + 0.1 * g.random(4)
    keys = []
    for k, f in enumerate(FRAMES):
        fov = (torch.tensor(fx[k], dtype=torch.float64), torch.tensor(fy[k], dtype=torch.float64)) if tensor_fov else (fx[k], fy[k])
        keys.append(SimpleNamespace(R=R[k], T=T[k], FoVx=fov[0], FoVy=fov[1], image_width=sizes[k][0], image_height=sizes[k][1],
                                    image_name="%06d" % f))
    return keys, R, T, fx, fy


def _expected(i, R, T, fx, fy):
    """frame i of the full path, by the issue's words"""
    j = max(k for k, f in enumerate(FRAMES) if f <= i)
    alpha = 1 - (i - FRAMES[j]) / (FRAMES[j + 1] - FRAMES[j])
    Ri = RotationSpline(FRAMES, Rotation.from_matrix(R))([i]).as_matrix()[0]
    return j, Ri, alpha * T[j] + (1 - alpha) * T[j + 1], alpha * fx[j] + (1 - alpha) * fx[j + 1], alpha * fy[j] + (1 - alpha) * fy[j + 1]


def test_every_frame_of_the_path():
    _, R, T, fx, fy = _keys()
    p = interpolate_poses(FRAMES, R, T, fx, fy, speed_up=1)
    assert p["frame"].tolist() == list(range(3, 15))
    for v in p.values():
        assert v.dtype == np.float64
    assert p["R"].shape == (12, 3, 3) and p["T"].shape == (12, 3) and p["fovx"].shape == (12,) and p["key"].shape == (12,)
    assert p["key"].tolist() == [0, 0, 0, 0, 1, 2, 2, 2, 2, 2, 2, 2]
    for n, i in enumerate(range(3, 15)):
        j, Ri, Ti, fxi, fyi = _expected(i, R, T, fx, fy)
        assert np.allclose(p["R"][n], Ri, rtol=0, atol=1e-12)
        assert np.allclose(p["T"][n], Ti, rtol=0, atol=1e-14)
        assert math.isclose(p["fovx"][n], fxi, rel_tol=1e-14) and math.isclose(p["fovy"][n], fyi, rel_tol=1e-14)
        assert np.allclose(p["R"][n] @ p["R"][n].T, np.eye(3), atol=1e-12)


def test_at_a_key_frame_the_pose_is_the_keys():
    _, R, T, fx, fy = _keys()
    p = interpolate_poses(FRAMES, R, T, fx, fy, speed_up=1)
    for k, f in enumerate(FRAMES[:-1]):       # the last key's frame is not part of the path: [frames[0], frames[-1])
        n = f - FRAMES[0]
        assert np.allclose(p["R"][n], R[k], rtol=0, atol=1e-12)
        assert np.array_equal(p["T"][n], T[k]) and p["fovx"][n] == fx[k] and p["fovy"][n] == fy[k]   # alpha = 1: 1 * a + 0 * b
    assert 15 not in p["frame"]


def test_in_between_the_blend_is_linear():
    _, R, T, fx, fy = _keys()
    p = interpolate_poses(FRAMES, R, T, fx, fy, speed_up=1)
    n = 5 - 3                                # frame 5: halfway between the keys at 3 and 7
    assert np.allclose(p["T"][n], 0.5 * (T[0] + T[1]), rtol=0, atol=1e-15) and math.isclose(p["fovx"][n], 0.5 * (fx[0] + fx[1]))
    n = 10 - 3                               # frame 10: 2 / 7 of the way from the key at 8 to the key at 15
    assert np.allclose(p["T"][n], T[2] + (T[3] - T[2]) * 2 / 7, rtol=0, atol=1e-14)


@pytest.mark.parametrize("speed_up,offset,most,want", [
    (4, 0, 300, [3, 7, 11]),
    (1, 0, 5, [3, 4, 5, 6, 7]),
    (2, 1, 3, [5, 7, 9]),
    (5, 2, 300, [13]),
    (4, 3, 300, []),                         # an offset past the end
    (4, 0, 0, []),
    (3, 1, 2, [6, 9]),
])
def test_the_path_is_sliced_as_stated(speed_up, offset, most, want):
    keys, R, T, fx, fy = _keys()
    p = interpolate_poses(FRAMES, R, T, fx, fy, speed_up=speed_up, max_frames=most, frame_offset=offset)
    assert p["frame"].tolist() == want == list(range(3, 15))[::speed_up][offset:offset + most]
    cams = interpolated_cameras(keys, speed_up=speed_up, max_frames=most, frame_offset=offset)
    assert [c.image_name for c in cams] == ["%06d" % i for i in want]
    full = interpolate_poses(FRAMES, R, T, fx, fy, speed_up=1)
    for n, i in enumerate(want):
        assert np.array_equal(p["R"][n], full["R"][i - 3]) and np.array_equal(p["T"][n], full["T"][i - 3])


def test_cameras_carry_the_poses():
    keys, R, T, fx, fy = _keys()
    p = interpolate_poses(FRAMES, R, T, fx, fy, speed_up=1)
    cams = scene.interpolated_cameras(keys, speed_up=1)
    assert len(cams) == 12 and all(isinstance(c, Camera) for c in cams)
    for n, c in enumerate(cams):
        assert c.image_name == "%06d" % (3 + n)
        assert np.array_equal(c.R, p["R"][n]) and np.array_equal(c.T, p["T"][n])
        w2c = torch.tensor(getWorld2View2(p["R"][n], p["T"][n]), dtype=torch.float32)
        assert torch.equal(c.world_view_transform, w2c.transpose(0, 1))
        assert float(c.FoVx) == np.float32(p["fovx"][n]) and float(c.FoVy) == np.float32(p["fovy"][n])
        key = keys[int(p["key"][n])]
        assert (c.image_width, c.image_height) == (key.image_width, key.image_height)
    assert (cams[5].image_width, cams[5].image_height) == (40, 60)     # frame 8: the third key's own size
    assert (cams[4].image_width, cams[4].image_height) == (36, 64)


def test_tensor_fovs_and_unsorted_keys():
    keys, R, T, fx, fy = _keys(tensor_fov=True)
    want = interpolated_cameras(keys, speed_up=1)
    shuffled = [keys[2], keys[0], keys[3], keys[1]]
    got = interpolated_cameras(shuffled, speed_up=1)
    assert [c.image_name for c in got] == [c.image_name for c in want]
    for a, b in zip(got, want):
        assert np.array_equal(a.R, b.R) and np.array_equal(a.T, b.T) and torch.equal(a.FoVx, b.FoVx)
    p = interpolate_poses(FRAMES, R, T, fx, fy, speed_up=1)
    assert np.array_equal(np.stack([c.T for c in got]), p["T"])


def test_what_is_refused():
    keys, R, T, fx, fy = _keys()
    with pytest.raises(ValueError):
        interpolated_cameras(keys[:1])
    with pytest.raises(ValueError):
        interpolate_poses([3], R[:1], T[:1], fx[:1], fy[:1])
    dup = [keys[0], keys[1], SimpleNamespace(**{**vars(keys[1])}), keys[3]]
    with pytest.raises(ValueError, match="increasing"):
        interpolated_cameras(dup)
    with pytest.raises(ValueError, match="increasing"):
        interpolate_poses([3, 7, 7, 15], R, T, fx, fy)
    with pytest.raises(ValueError, match="increasing"):
        interpolate_poses([3, 8, 7, 15], R, T, fx, fy)
    # names sort as strings: "10" < "9", so the frame numbers 10, 9 are not increasing
    odd = [SimpleNamespace(**{**vars(keys[0]), "image_name": "9"}), SimpleNamespace(**{**vars(keys[1]), "image_name": "10"})]
    with pytest.raises(ValueError, match="increasing"):
        interpolated_cameras(odd)
