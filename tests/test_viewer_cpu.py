"""CPU checks of the viewer camera and video recording: the viewer header's layout and symbols, argument refusals before any
launch, the look-at camera model against the depth oracle, RecordVideo's trigger / length / naming on a stub env, the animated PNG
writer, and the viewer config defaults."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT
from wheeledlab_amd import _abi as A

HEADER = os.path.join(ROOT, "include", "wheeledlab_amd_viewer.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    return A.load()


def test_viewer_params_layout_matches_header(tmp_path):
    fields = [n for n, _ in A.WlViewerParams._fields_]
    probe = tmp_path / "probe.c"
    body = " ".join(f'printf("%zu ", offsetof(WlViewerParams, {n}));' for n in fields)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wheeledlab_amd_viewer.h"\n'
                     f'int main(){{{body} printf("%zu %d %d %d %d\\n", sizeof(WlViewerParams), (int)WL_VIEWER_VERSION, (int)WL_VIEWER_PLANE,'
                     ' (int)WL_VIEWER_HEIGHTFIELD, (int)WL_VIEWER_TILE); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [getattr(A.WlViewerParams, n).offset for n in fields] + [C.sizeof(A.WlViewerParams), A.WL_VIEWER_VERSION, A.VIEWER_PLANE,
                                                                     A.VIEWER_HEIGHTFIELD, A.VIEWER_TILE]
    assert got == want


def test_viewer_symbols_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wl_[a-z0-9_]+)\s*\(", src))
    assert declared == set(A.VIEWER_SIGNATURES)
    assert not declared & set(A.SIGNATURES)      # outside the drop-in step boundary
    lib = _lib()
    for name in declared:
        assert getattr(lib, name).argtypes is not None
    assert lib.wl_viewer_version() == A.WL_VIEWER_VERSION


def _params(w=64, h=48, **kw):
    from wheeledlab_amd.viewer import viewer_params
    p = viewer_params(w, h, (4.0, -4.0, 4.0), (0.0, 0.0, 0.0))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_viewer_refuses_bad_arguments_without_a_gpu():
    lib = _lib()
    assert lib.wl_viewer_scratch_bytes(0, 10, 10) < 0 and lib.wl_viewer_scratch_bytes(10, -1, 10) < 0
    assert lib.wl_viewer_scratch_bytes(10, 10, 0) < 0 and lib.wl_viewer_scratch_bytes(9000, 10, 10) < 0
    need = lib.wl_viewer_scratch_bytes(64, 48, 8)
    assert need > 0
    fake = 1 << 20          # never dereferenced: every call below is refused before any launch
    bufs = A.WlEnvBuffers(fake, fake, None, fake, 64, 8, 0, 1, 0, 0)
    hf = A.WlHeightField(fake, 16, 16, -1.0, -1.0, 0.1, 0.0, 2.0 ** -13, None)

    def call(p=None, b=bufs, h=None, pyr=None, m=None, scratch=fake, nbytes=need, rgb=fake):
        return lib.wl_viewer_render(C.byref(p or _params()), C.byref(b), C.byref(h) if h is not None else None, pyr,
                                    C.byref(m) if m is not None else None, scratch, nbytes, rgb, None, None, None)
    assert call(rgb=None) == -1                                        # no rgb
    assert call(p=_params(w=0)) == -1 and call(p=_params(h=-3)) == -1   # sizes <= 0
    assert call(b=A.WlEnvBuffers(fake, fake, None, fake, 64, 0, 0, 1, 0, 0)) == -1
    assert call(nbytes=need - 1) == -1                                 # scratch too small
    assert call(scratch=None) == -1
    assert call(p=_params(ground=A.VIEWER_HEIGHTFIELD), h=hf) == -1     # heightfield without its pyramid
    assert call(p=_params(ground=A.VIEWER_HEIGHTFIELD)) == -1          # heightfield mode without the field
    assert call(h=hf, pyr=fake) == -1                                  # a field handed to the plane mode
    assert call(p=_params(checker=0.0)) == -1                          # no map and no checker
    assert call(m=A.WlTravMap(fake, None, 40, 60, 0, 0.5, 0.5, None)) == -1   # a non-square map (lookups would leave it)
    assert call(p=_params(far_clip=0.0)) == -1 and call(p=_params(fx=float("nan"))) == -1
    assert call(scratch=fake + 4) == -3                                # misaligned scratch


def test_look_at_plane_depth_equals_depth_oracle():
    """the camera model: a ground pixel's depth from the reference's plane equals oracle.depth.depth() for a root pose at `eye` with
    the look-at rotation and cam_pos = 0 (flat field at z = 0, the outside plane z = 0 too)"""
    import viewer_reference as VR
    from oracle import depth as OD
    from wheeledlab_amd.viewer import look_at
    for eye, lookat in (((4.0, -4.0, 4.0), (0.0, 0.0, 0.0)), ((20.0, -20.0, 20.0), (0.0, 0.0, 0.0)), ((40.0, 0.0, 45.0), (0.0, 0.0, -3.0)),
                        ((0.3, 0.2, 9.0), (0.3, 0.2, 0.0))):        # the last looks straight down: y is the up vector
        p = _params(w=80, h=60, far_clip=200.0)
        pos, quat = look_at(eye, lookat)
        p.cam_pos[:], p.cam_quat[:] = list(map(float, pos)), list(map(float, quat))
        rgb, depth, ids = VR.render(p, np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32))
        cam = SimpleNamespace(cam_pos=(0.0, 0.0, 0.0), fx=p.fx, fy=p.fy, cx=p.cx, cy=p.cy)
        field = (np.zeros((41, 41), np.float32), -20.0, -20.0, 1.0)
        want = OD.depth(cam, pos[None], quat[None], field, 200.0, img_h=60, img_w=80)[0]
        np.testing.assert_allclose(depth, want, rtol=2e-5, atol=2e-5)
        # the optical axis is lookat - eye: the centre ray hits the plane where the look-at line does
        f = np.asarray(lookat, float) - np.asarray(eye, float)
        R = np.array([[1 - 2 * (quat[2] ** 2 + quat[3] ** 2)], [2 * (quat[1] * quat[2] + quat[3] * quat[0])],
                      [2 * (quat[1] * quat[3] - quat[2] * quat[0])]])[:, 0]
        np.testing.assert_allclose(R, f / np.linalg.norm(f), atol=1e-6)
        assert (ids[depth < 200.0] == -1).all() and (ids[depth >= 200.0] == -2).all()


class _StubEnv:
    """a base env as far as RecordVideo is concerned: a step counter, frame hooks, a frame"""
    def __init__(self, h=6, w=10):
        self.common_step_counter, self._frame_hooks, self.metadata = 0, [], {"render_fps": 5.0}
        self.h, self.w = h, w
        self.rendered = []

    @property
    def unwrapped(self):
        return self

    def add_frame_hook(self, hook):
        self._frame_hooks.append(hook)

    def remove_frame_hook(self, hook):
        self._frame_hooks.remove(hook)

    def render_frame(self, resolution=None):
        import torch
        self.rendered.append(self.common_step_counter)
        return torch.full((self.h, self.w, 3), self.common_step_counter % 256, dtype=torch.uint8)

    def step(self, a=None):
        self.common_step_counter += 1
        for h in list(self._frame_hooks):
            h(self)


def _read_apng(path):
    """-> (frames [k, H, W, 3], acTL num_frames): a minimal parser of what video.ApngWriter writes (filter type 0 rows)"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    k, chunks = 8, []
    while k < len(data):
        n, kind = struct.unpack(">I4s", data[k:k + 8])
        body = data[k + 8:k + 8 + n]
        assert struct.unpack(">I", data[k + 8 + n:k + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff
        chunks.append((kind, body))
        k += 12 + n
    kinds = [c[0] for c in chunks]
    assert kinds[0] == b"IHDR" and kinds[1] == b"acTL" and kinds[-1] == b"IEND"
    w, h, depth, ctype = struct.unpack(">IIBB", chunks[0][1][:10])
    assert (depth, ctype) == (8, 2)
    n_frames = struct.unpack(">II", chunks[1][1])[0]
    frames, seqs = [], []
    for kind, body in chunks:
        if kind == b"fcTL":
            seqs.append(struct.unpack(">I", body[:4])[0])
        elif kind in (b"IDAT", b"fdAT"):
            if kind == b"fdAT":
                seqs.append(struct.unpack(">I", body[:4])[0])
                body = body[4:]
            rows = np.frombuffer(zlib.decompress(body), np.uint8).reshape(h, 1 + 3 * w)
            assert (rows[:, 0] == 0).all()
            frames.append(rows[:, 1:].reshape(h, w, 3))
    assert seqs == list(range(len(seqs)))           # one sequence over fcTL and fdAT chunks
    return np.stack(frames) if frames else np.zeros((0, h, w, 3), np.uint8), n_frames


def test_record_video_trigger_and_length(tmp_path):
    from wheeledlab_amd.video import RecordVideo
    env = _StubEnv()
    I, L = 10, 4
    rec = RecordVideo(env, video_folder=str(tmp_path), step_trigger=lambda s: s % I == 0, video_length=L, name_prefix="rl-video",
                      disable_logger=True, writer="apng")
    # the runner's question: would the next K steps need frames?
    assert rec.wants_frames(0, 3)            # a clip is open
    for _ in range(25):
        env.step()
    assert not rec.recording and not rec.wants_frames(env.common_step_counter, 4) and rec.wants_frames(env.common_step_counter, 5)
    rec.close()
    assert env.rendered == [0, 1, 2, 3, 10, 11, 12, 13, 20, 21, 22, 23]
    names = sorted(os.listdir(tmp_path))
    assert names == ["rl-video-step-0.png", "rl-video-step-10.png", "rl-video-step-20.png"]
    for name, k0 in (("rl-video-step-0.png", 0), ("rl-video-step-10.png", 10), ("rl-video-step-20.png", 20)):
        frames, n = _read_apng(os.path.join(tmp_path, name))
        assert n == L and len(frames) == L
        assert [int(f[0, 0, 0]) for f in frames] == list(range(k0, k0 + L))     # the frame of counter k0 + i, in order


def test_record_video_never_triggered_writes_nothing(tmp_path):
    from wheeledlab_amd.video import RecordVideo
    env = _StubEnv()
    rec = RecordVideo(env, video_folder=str(tmp_path / "v"), step_trigger=lambda s: False, video_length=3, writer="apng")
    for _ in range(20):
        env.step()
    assert not rec.wants_frames(env.common_step_counter, 100)
    rec.close()
    assert env.rendered == [] and os.listdir(tmp_path / "v") == [] and env._frame_hooks == []


def test_apng_round_trip_is_byte_exact(tmp_path):
    from wheeledlab_amd.video import ApngWriter
    rng = np.random.RandomState(0)
    frames = rng.randint(0, 256, (5, 13, 17, 3)).astype(np.uint8)
    w = ApngWriter(str(tmp_path / "a.png"), 17, 13, fps=50)
    for f in frames:
        w.write(f)
    w.close()
    got, n = _read_apng(str(tmp_path / "a.png"))
    assert n == 5
    np.testing.assert_array_equal(got, frames)


def test_viewer_cfg_defaults_and_video_off_by_default():
    from wheeledlab_amd.configs import LogConfig
    from wheeledlab_amd.envs.managers_cfg import ViewerCfg
    v = ViewerCfg()
    assert list(v.eye) == [7.5, 7.5, 7.5] and list(v.lookat) == [0.0, 0.0, 0.0]
    assert tuple(v.resolution) == (1280, 720) and v.origin_type == "world" and v.env_index == 0 and v.asset_name == "robot"
    log = LogConfig()
    assert log.video is False and tuple(log.video_resolution) == (1280, 720)
    from wheeledlab_amd.envs.manager_based_rl_env import ManagerBasedRLEnv
    assert "rgb_array" in ManagerBasedRLEnv.metadata["render_modes"] and None in ManagerBasedRLEnv.metadata["render_modes"]


def test_look_at_intrinsics():
    from wheeledlab_amd.viewer import intrinsics
    fx, fy, cx, cy = intrinsics(1280, 720)
    assert fx == fy and abs(fx - 640 / np.tan(np.radians(30))) < 1e-9 and (cx, cy) == (640, 360)
