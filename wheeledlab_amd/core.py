"""DriftBatch, ElevBatch, VisualBatch, VisualDepthBatch: device buffers of one shard of a task's envs + thin calls into the C ABI.

PyTorch is plumbing here: it owns the HBM allocations and the stream; every kernel is ours (csrc/*.hip).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _abi as A
from .params import drift_params


def stadium_reference_poses(u: torch.Tensor, track_radius: float = 0.8, straight: float = 0.8) -> torch.Tensor:
    """Pre-sampled reset poses on the stadium centre line: arclength u*L -> (x, y, yaw rad), [3, P].
    Follows reset_root_state_along_track.generate_reference_poses (wheeledlab_tasks/drifting/mdp/events.py:33-100):
    four pieces -- right straight (yaw 90 deg), top arc, left straight (yaw 270 deg), bottom arc."""
    r, s = track_radius, straight
    d = u.double() * (2.0 * math.pi * r + 4.0 * s)
    x, y, yaw = torch.empty_like(d), torch.empty_like(d), torch.empty_like(d)
    b1, b2, b3 = 2 * s, 2 * s + math.pi * r, 4 * s + math.pi * r
    m = d < b1
    x[m], y[m], yaw[m] = r, d[m] - s, math.pi / 2
    m = (d >= b1) & (d < b2)
    a = (d[m] - b1) / r
    x[m], y[m], yaw[m] = r * torch.cos(a), s + r * torch.sin(a), math.pi / 2 + a
    m = (d >= b2) & (d < b3)
    x[m], y[m], yaw[m] = -r, s - (d[m] - b2), 1.5 * math.pi
    m = d >= b3
    a = (d[m] - b3) / r
    x[m], y[m], yaw[m] = -r * torch.cos(a), -s - r * torch.sin(a), 1.5 * math.pi + a
    return torch.stack([x, y, yaw]).float()


def apply_startup_events(lib, bufs: "A.WlEnvBuffers", su, seed: int, stream, randomize: bool = True):
    """startup-mode events (domain randomisation, applied once): bucketed wheel friction
    (isaaclab randomize_rigid_body_material), throttle damping (randomize_actuator_gains, "abs"), base mass
    (randomize_rigid_body_mass, "add" onto the chassis mass).  Reference configs: mushr_drift_env_cfg.py:98-119,145-154;
    elevation cfg :387-407; visual cfg :264-299.  One launch of wl_startup_randomize: the draws are keyed by the GLOBAL
    env id (bufs.env_offset + e), so a sharded run holds the same parameter sets as the one big batch."""
    sp = A.WlStartupParams((C.c_float * 2)(*su.wheel_mu_s), (C.c_float * 2)(*su.wheel_mu_d), int(su.mu_buckets),
                           int(bool(su.mu_consistent)), (C.c_float * 2)(*su.damping), float(su.chassis_mass),
                           (C.c_float * 2)(*su.mass_add), int(bool(randomize)), (C.c_float * 2)(*getattr(su, "wheel_mass", (0.0, 0.0))))
    A.check(lib.wl_startup_randomize(C.byref(sp), C.byref(bufs), int(seed), stream), "wl_startup_randomize")


def _canonical_device(device) -> torch.device:
    """torch.device with its index filled in: 'cuda' and 'cuda:0' name the same GPU but compare unequal"""
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    return d


def pair_table(codes: torch.Tensor) -> torch.Tensor:
    """WlHeightField.pair as the header defines it: pair[j][i] = code[j][i] (low half) | code[min(j + 1, ny - 1)][i] << 16, int32
    [ny, nx] (what wl_heightfield_pairs builds on the device; here in torch, for host-side fields and as the test's definition)"""
    c = codes.to(torch.int32)
    up = torch.cat([c[1:], c[-1:]], 0)
    return ((c & 0xffff) | (up << 16)).to(torch.int32).contiguous()


class DeviceHeightField:
    """A heightfield resident on the device as the kernels read it (WlHeightField, ABI 21): 16-bit height codes [ny, nx] and the
    vertical scale, z = code * z_scale.  `heightfield` is `(height, x0, y0, cell)` with float heights (quantised: terrain.
    quantize_heights' rule, z_scale 2^-13 m unless the range needs more) or `(codes int16, x0, y0, cell, z_scale)`, arrays or
    tensors; or another DeviceHeightField on the same device (shared).  `.heights`: the decoded fp32 grid -- exactly the values
    every kernel sees (what tests hand to the oracle).  `outside_z`: the height of the plane beyond the grid (what the contact samplers
    and the depth walk meet there); None keeps a shared field's own, else 0.  The field owns every table derived from the codes,
    one of each for all its views: `pairs`, `heights` and `pyramid`, and every FlatPatches found on it; after editing `codes` in
    place, refresh() them.  A field made by
    generate_heightfield remembers its TerrainGeneratorCfg (`generator`) and can be drawn again in place: regenerate()."""

    def __init__(self, heightfield, device, outside_z: float | None = None):
        from .terrain import default_z_scale
        self.device = _canonical_device(device)
        if isinstance(heightfield, DeviceHeightField):
            src = heightfield
            if src.device != self.device:
                raise ValueError(f"a DeviceHeightField lives on {src.device}; it cannot be shared with {self.device}")
            self.codes, self.z_scale, self.heights, self.pairs = src.codes, src.z_scale, src.heights, src.pairs
            self.x0, self.y0, self.cell = src.x0, src.y0, src.cell
            self._shared = src._shared
            outside_z = src.outside_z if outside_z is None else outside_z
        else:
            h, x0, y0, cell, *rest = heightfield
            h = torch.as_tensor(h)
            if h.dtype == torch.int16:
                if not rest:
                    raise ValueError("int16 height codes need their z_scale: (codes, x0, y0, cell, z_scale)")
                self.codes, self.z_scale = h.contiguous().to(self.device), float(rest[0])
            else:
                h = h.to(self.device, torch.float64)
                if not bool(torch.isfinite(h).all()):
                    raise ValueError("heightfield with non-finite heights")
                hmax = float(h.abs().max()) if h.numel() else 0.0
                self.z_scale = float(rest[0]) if rest else default_z_scale(hmax)
                if rest and math.isfinite(self.z_scale) and self.z_scale > 0 and hmax > 32767 * self.z_scale:
                    # (the default scale widens itself; an explicit one that cannot hold the heights would flatten them silently)
                    raise ValueError(f"heights up to {hmax:g} m do not fit 16-bit codes of z_scale {self.z_scale:g} m "
                                     f"(+-{32767 * self.z_scale:g} m): pass a larger z_scale or none")
                self.codes = torch.clamp(torch.round(h / self.z_scale), -32767, 32767).to(torch.int16).contiguous() if (
                    math.isfinite(self.z_scale) and self.z_scale > 0) else torch.zeros((0,), dtype=torch.int16)
            if not (math.isfinite(self.z_scale) and self.z_scale > 0) or self.codes.dim() != 2:
                raise ValueError("heightfield: a [ny, nx] grid and a positive, finite z_scale")
            self.x0, self.y0, self.cell = float(x0), float(y0), float(cell)
            # the decoded grid and the row-pair table the height scan gathers from (WlHeightField.pair, ABI 23): filled by refresh()
            self.heights = torch.empty(self.codes.shape, dtype=torch.float32, device=self.device)
            self.pairs = torch.empty(self.codes.shape, dtype=torch.int32, device=self.device)
            # what every view of these buffers shares: the generator's config (None: not generated), the bound pyramid (None: no ray cast yet)
            # and the flat-patch sets found on it (weak references: a set lives as long as its owner)
            self._shared = {"generator": None, "pyramid": None, "patches": []}
        self.outside_z = float(0.0 if outside_z is None else outside_z)
        ny, nx = self.codes.shape
        self.struct = A.WlHeightField(self.codes.data_ptr(), nx, ny, self.x0, self.y0, self.cell, self.outside_z, self.z_scale, self.pairs.data_ptr())
        if not isinstance(heightfield, DeviceHeightField):
            self.refresh()

    def _build(self, fn: str, table: torch.Tensor):
        """a derived table from the codes, on the current stream"""
        A.check(getattr(A.load(), fn)(C.byref(self.struct), table.data_ptr(), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), fn)

    @property
    def pyramid(self) -> torch.Tensor:
        """the bound pyramid the depth walk, the lidar scan and the viewer descend (float32 [wl_heightfield_pyramid_floats], packed
        words): built at the first access, ONE for all views -- the builder reads no outside_z, the walks apply their view's own"""
        if self._shared["pyramid"] is None:
            if self.device.type != "cuda":
                raise A.HipExtensionMissing("the bound pyramid needs a field on a HIP device (device='cuda:N'); there is no CPU path")
            ny, nx = self.codes.shape
            n_f = int(A.load().wl_heightfield_pyramid_floats(nx, ny))
            if n_f <= 0:
                raise A.WlError(f"heightfield of {nx} x {ny} points is outside the pyramid's range")
            # (zeros: the builder leaves the padding between the levels alone -- equal fields give equal buffers, word for word)
            pyr = torch.zeros(n_f, dtype=torch.float32, device=self.device)
            self._build("wl_heightfield_build_pyramid", pyr)
            self._shared["pyramid"] = pyr
        return self._shared["pyramid"]

    def refresh(self):
        """Bring every derived table in line with `codes` as they are now, in place (no address moves): `pairs`, `heights` and, once
        built, the pyramid.  Run it after editing `codes` in place: nothing detects such an edit, and the kernels read the tables."""
        if self.device.type == "cuda":
            self._build("wl_heightfield_pairs", self.pairs)
        else:
            self.pairs.copy_(pair_table(self.codes))
        torch.mul(self.codes.to(torch.float32), torch.tensor(self.z_scale, dtype=torch.float32, device=self.device), out=self.heights)
        if self._shared["pyramid"] is not None:
            self._build("wl_heightfield_build_pyramid", self._shared["pyramid"])
        if self._shared["patches"]:       # (no flat patches on the field: nothing is launched for them)
            live = [r for r in self._shared["patches"] if r() is not None]
            self._shared["patches"][:] = live
            for r in live:
                r().find()
        return self

    def as_tuple(self):
        """(decoded heights, x0, y0, cell): the form the oracle's functions take"""
        return self.heights, self.x0, self.y0, self.cell

    @property
    def generator(self):
        """the TerrainGeneratorCfg the codes were last generated from (None: not a generated field)"""
        return self._shared["generator"]

    def regenerate(self, cfg_or_seed=None):
        """Draw the field again IN PLACE from a TerrainGeneratorCfg, or from the current one under another seed (an int; None: the
        same seed): new codes into the same device buffers (wl_terrain_generate), then refresh() -- every WlHeightField and pyramid
        pointer a batch holds stays valid, and nothing that reads the field afterwards sees the old one.  The new config must give
        the same lattice (points, placement, vertical scale).  Cars stand where they stood: reset them (env.regenerate_terrain does)."""
        from .envs import terrain_gen_cfg as G
        if self.device.type != "cuda":
            raise A.HipExtensionMissing("regenerate needs a field on a HIP device (device='cuda:N'); there is no CPU path")
        cfg = self.generator
        if isinstance(cfg_or_seed, int) and not isinstance(cfg_or_seed, bool):
            if cfg is None:
                raise ValueError("regenerate(seed) needs a generated field (core.generate_heightfield); pass a TerrainGeneratorCfg")
            cfg = cfg.replace(seed=int(cfg_or_seed))
        elif cfg_or_seed is not None:
            cfg = cfg_or_seed
        if cfg is None:
            raise ValueError("regenerate() of a field that was not generated needs a TerrainGeneratorCfg")
        geo = G.lattice(cfg)
        ny, nx = self.codes.shape
        if (geo["nx"], geo["ny"]) != (nx, ny) or (geo["x0"], geo["y0"], geo["cell"], geo["z_scale"]) != (self.x0, self.y0, self.cell, self.z_scale):
            raise ValueError(f"regenerate: the config gives a lattice of {geo['nx']} x {geo['ny']} points at ({geo['x0']:g}, {geo['y0']:g}), "
                             f"cell {geo['cell']:g} m, z_scale {geo['z_scale']:g} m; the field is {nx} x {ny} at ({self.x0:g}, {self.y0:g}), "
                             f"cell {self.cell:g} m, z_scale {self.z_scale:g} m -- build a new field instead")
        _launch_terrain_generator(cfg, self.codes)
        self._shared["generator"] = cfg
        # _field_key tells snapshots of this tensor (fields from a TUPLE holding it, which nobody refreshes) apart by its version
        # counter, which a kernel write through data_ptr() does not touch: bump it by hand
        torch.autograd.graph.increment_version(self.codes)
        return self.refresh()


def _launch_terrain_generator(cfg, codes: torch.Tensor):
    """validate the config's descriptor table on the host (wl_terrain_gen_check), upload it and generate into `codes`"""
    import numpy as np

    from .envs import terrain_gen_cfg as G
    lib = A.load()
    p, table = G.gen_params(cfg), np.ascontiguousarray(G.tile_table(cfg))
    if lib.wl_terrain_gen_check(C.byref(p), table.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError("TerrainGeneratorCfg resolves to a grid or a sub-terrain outside the generator's range "
                         "(include/wheeledlab_amd_terrain.h: sizes, level ranges within +-32767 codes, at most 64 obstacles)")
    if codes.device.type != "cuda" or codes.dtype != torch.int16 or not codes.is_contiguous() or tuple(codes.shape) != (p.ny, p.nx):
        raise ValueError(f"the generator writes contiguous int16 codes [{p.ny}, {p.nx}] on a HIP device")
    tiles = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(codes.device)
    A.check(lib.wl_terrain_generate(C.byref(p), tiles.data_ptr(), codes.data_ptr(),
                                    C.c_void_p(torch.cuda.current_stream(codes.device).cuda_stream)), "wl_terrain_generate")


def generate_heightfield(cfg, device="cuda:0", outside_z: float | None = None) -> DeviceHeightField:
    """A procedural terrain (envs.terrain_gen_cfg.TerrainGeneratorCfg) generated on the device: the codes are allocated there and
    written by wl_terrain_generate, the pair table by wl_heightfield_pairs -- nothing but the tile descriptors (64 bytes each)
    crosses the bus.  -> a DeviceHeightField that ElevBatch / VisualDepthBatch / DepthCamera take as `heightfield`, and whose
    regenerate() draws it again in place.  `outside_z`: the plane beyond the lattice, 0 unless given (as for every other field)."""
    from .envs import terrain_gen_cfg as G
    dev = _canonical_device(device)
    if dev.type != "cuda":
        raise A.HipExtensionMissing("generate_heightfield needs a HIP device (device='cuda:N'); there is no CPU path")
    geo = G.lattice(cfg)
    codes = torch.empty((geo["ny"], geo["nx"]), dtype=torch.int16, device=dev)
    _launch_terrain_generator(cfg, codes)
    hf = DeviceHeightField((codes, geo["x0"], geo["y0"], geo["cell"], geo["z_scale"]), dev, outside_z)
    hf._shared["generator"] = cfg
    return hf


def mesh_heightfield(vertices, faces, cell: float, device="cuda:0", lattice=None, fill_z: float = 0.0, stats: dict | None = None):
    """Rasterise a triangle mesh into a height lattice on the device (include/wheeledlab_amd_terrain.h: wl_mesh_raster): at each
    lattice point the highest triangle whose xy projection contains it, `fill_z` where none does -- what a height scanner casting
    straight down returns.  `vertices` float [V, 3] (world, metres) and `faces` int [F, 3], arrays or tensors; `lattice` = (x0, y0,
    nx, ny), or None for the mesh's xy bounds on multiples of `cell`.  -> (heights float32 [ny, nx] on `device`, x0, y0, cell): the
    tuple DeviceHeightField, ElevBatch(heightfield=...), VisualDepthBatch(heightfield=...) and scene.terrain.heightfield take.
    Raises ValueError for faces with an index outside [0, V) or a non-finite vertex (one synchronisation: the launch's status).
    `stats`: a dict that receives the launch's status words (invalid, binned, big, entries: WL_TERRAIN_STATUS_WORDS)."""
    dev = _canonical_device(device)
    v = torch.as_tensor(vertices).to(dev, torch.float32).reshape(-1, 3).contiguous()
    f = torch.as_tensor(faces).to(dev).reshape(-1, 3)
    if f.dtype.is_floating_point or f.dtype == torch.bool:
        raise ValueError("faces must be integer vertex indices")
    if f.numel() and (int(f.min()) < -2 ** 31 or int(f.max()) >= 2 ** 31):
        raise ValueError("face indices beyond int32")
    f = f.to(torch.int32).contiguous()
    c32 = float(torch.tensor(cell, dtype=torch.float32))
    if not (math.isfinite(c32) and c32 > 0):
        raise ValueError("cell must be positive and finite")
    if lattice is None:
        if v.shape[0] == 0:
            raise ValueError("an empty mesh has no bounds: pass lattice=(x0, y0, nx, ny)")
        lo, hi = v[:, :2].double().min(0).values.tolist(), v[:, :2].double().max(0).values.tolist()
        if not all(math.isfinite(a) for a in lo + hi):
            raise ValueError("mesh with non-finite vertex coordinates")
        x0, y0 = (float(torch.tensor(c32 * math.floor(a / c32), dtype=torch.float32)) for a in lo)
        nx, ny = (max(2, math.ceil((b - a) / c32) + 1) for a, b in zip((x0, y0), hi))
    else:
        x0, y0, nx, ny = lattice
        x0, y0, nx, ny = float(torch.tensor(x0, dtype=torch.float32)), float(torch.tensor(y0, dtype=torch.float32)), int(nx), int(ny)
    lib = A.load()
    if not math.isfinite(float(fill_z)):
        raise ValueError("fill_z must be finite")
    fits = max(abs(nx), abs(ny), f.shape[0], v.shape[0]) < 2 ** 31
    need = lib.wl_mesh_raster_scratch_bytes(f.shape[0], nx, ny) if fits else -1
    if need <= 0:
        raise ValueError(f"a lattice of {nx} x {ny} points (2 .. {A.TERRAIN_MAX_SIDE - 1} each, at most 2^31 - 1 in all) for "
                         f"{f.shape[0]} faces is out of range")
    p = A.WlMeshRasterParams(x0, y0, c32, nx, ny, float(fill_z))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    heights = torch.empty((ny, nx), dtype=torch.float32, device=dev)
    status = torch.zeros(A.TERRAIN_STATUS_WORDS, dtype=torch.int32, device=dev)
    A.check(lib.wl_mesh_raster(C.byref(p), v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], scratch.data_ptr(), need, heights.data_ptr(),
                               status.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "wl_mesh_raster")
    words = status.tolist()
    if stats is not None:
        stats.update(zip(("invalid", "binned", "big", "entries"), words))
    bad = words[0]
    if bad:
        raise ValueError(f"{bad} of {f.shape[0]} faces have a vertex index outside [0, {v.shape[0]}) or a non-finite vertex")
    return heights, x0, y0, c32


def ring_plan(step0: int, n_steps: int, slots: int):
    """How a persistent launch of `n_steps` steps from step `step0` runs on a metric ring of `slots` slots.  The launch folds all
    its steps into slot step0 % R and clears slot (step0 + n) % R for its successor.  Returns (segments, zero):
    segments -- the launches as (first step, steps): [(0, n)], or [(0, 1), (1, n - 1)] when n is a multiple of R: those two
    slots are then the same and the C ABI refuses the launch (WL_EINVAL).  Like n single steps, the split leaves the ring without
    the first step's counts (a ring of R slots holds R - 1 steps);
    zero -- the slots the host clears before the launches: those of the steps a launch folds away, which would otherwise keep
    the counts of an earlier pass over the ring."""
    if slots <= 1 or n_steps <= 1:
        return [(0, n_steps)], []
    segments = [(0, 1), (1, n_steps - 1)] if n_steps % slots == 0 else [(0, n_steps)]
    zero = sorted({(step0 + k0 + i) % slots for k0, k in segments for i in range(1, k)})
    return segments, zero


class _EnvBatch:
    """What every task's batch holds: n envs resident on one GPU as a SoA state matrix [S_COUNT, stride] (fp32), the per-step
    output rows, the episode-metric accumulators and the WlEnvBuffers / WlStepOut structs that hand them to the C ABI.  A task
    names its C entry points (_C_*) and sets `_args`: WlEnvBuffers and the task's own structs, by reference -- the arguments
    after the params of every reset / step / rollout call.

    `metrics_raw` is what the kernels add into: [slots][WL_M_SHARDS][WL_M_COUNT].  `metrics` is the logical value (sum over the
    shards): [WL_M_COUNT] for one accumulator, [slots][WL_M_COUNT] for a ring; a fresh tensor per read."""

    OBS_DIM: int
    LANES = (0, 1, 4)              # the step-kernel forms set_lanes() accepts
    _C_RESET = _C_STEP = _C_ROLLOUT = _C_PERSISTENT = None
    _PERSISTENT_NEEDS_ROWS = True  # the persistent kernel writes step k's observation while step k + 1 runs
    pose_epoch = 0       # bumped by everything that moves cars WITHOUT advancing step_count (resets, plugin pose writes)
    _out_key = None
    _ring_split_warned = False

    def __init__(self, n_envs: int, device, params, seed: int, env_offset: int, metrics_slots: int, ref_table=None):
        self.lib = A.load()  # raises HipExtensionMissing -- no fallback
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise A.HipExtensionMissing(f"{type(self).__name__} needs a HIP device (device='cuda:N'); there is no CPU path")
        self.n = int(n_envs)
        self.stride = ((self.n + 63) // 64) * 64
        self.p, self.seed, self.env_offset, self.step_count = params, int(seed), int(env_offset), 0
        dev = self.device
        self.state = torch.zeros(A.S_COUNT, self.stride, dtype=torch.float32, device=dev)
        self.episode_len = torch.zeros(self.stride, dtype=torch.int32, device=dev)
        self.metrics_slots = int(metrics_slots)
        self.metrics_raw = torch.zeros(self.metrics_slots, A.M_SHARDS, A.M_COUNT, dtype=torch.float32, device=dev)
        self.obs = torch.zeros(self.n, self.OBS_DIM, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(self.n, dtype=torch.float32, device=dev)
        # torch.bool is one byte holding 0 / 1: the kernel's uint8 outputs land in it directly
        self.terminated = torch.zeros(self.n, dtype=torch.bool, device=dev)
        self.truncated = torch.zeros(self.n, dtype=torch.bool, device=dev)
        self.dones = torch.zeros(self.n, dtype=torch.long, device=dev)   # terminated | truncated, as RSL-RL consumes it
        if ref_table is not None:
            self.ref_table = ref_table.to(dev)
        self._bufs = A.WlEnvBuffers(self.state.data_ptr(), self.episode_len.data_ptr(),
                                    None if ref_table is None else self.ref_table.data_ptr(), self.metrics_raw.data_ptr(),
                                    self.stride, self.n, self.env_offset, self.metrics_slots, 0, 0)
        self._out = A.WlStepOut(self.obs.data_ptr(), self.reward.data_ptr(), self.terminated.data_ptr(),
                                self.truncated.data_ptr(), self.dones.data_ptr())
        self._args = (C.byref(self._bufs),)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def metrics(self) -> torch.Tensor:
        m = self.metrics_raw.sum(1)
        return m[0] if self.metrics_slots == 1 else m

    def read_metrics(self, zero: bool = True) -> torch.Tensor:
        m = self.metrics
        if zero:
            self.metrics_raw.zero_()
        return m

    def touch_pose(self):
        """anything cached per env.step() from the poses (the scene camera's render) is stale after this"""
        self.pose_epoch = self.pose_epoch + 1

    def set_flags(self, flags: int = 0):
        """WlEnvBuffers.flags (_abi.FLAG_*): force an instantiation the launchers otherwise pick from the batch size -- the
        streaming (non-temporal store) forms or the cache-allocating forms.  0 = by size.  What the tests use to run the large-batch forms at small sizes (and vice versa)."""
        self._bufs.flags = int(flags)

    def set_lanes(self, lanes: int = 0):
        """step-kernel form, one of LANES: 0 = by env count (quad up to 32 768 envs; drift: lane form with packed axles up to
        262 144, with the scalar wheel loop beyond), 1 = lane per env (drift: packed axles), 2 = drift's lane form with the scalar
        wheel loop, 4 = quad per env"""
        assert lanes in self.LANES
        self._bufs.lanes = lanes

    def set_dones_output(self, on: bool = True):
        """the int64 `dones` row (terminated | truncated as RSL-RL's runner consumes it, + 8 B per env-step) of step() /
        in-place rollouts on or off; callers that read the two byte rows do not need it"""
        self._out.dones = self.dones.data_ptr() if on else None

    def reset(self, mask: torch.Tensor | None = None):
        self.touch_pose()
        m = None if mask is None else mask.to(torch.uint8).contiguous()
        A.check(getattr(self.lib, self._C_RESET)(C.byref(self.p), *self._args, None if m is None else m.data_ptr(), self.seed,
                                                 self.step_count, self._stream()), self._C_RESET)

    def _actions(self, actions: torch.Tensor) -> torch.Tensor:
        if actions.dtype != torch.float32 or not actions.is_contiguous() or actions.shape != (self.n, 2):
            actions = actions.to(torch.float32).reshape(self.n, 2).contiguous()
        return actions

    def step(self, actions: torch.Tensor):
        """actions [n, 2] -> (obs [n, OBS_DIM], reward [n], terminated [n], truncated [n]): the batch's own rows (views)"""
        return self._step(actions)

    def _step(self, actions, *after_actions):
        A.check(getattr(self.lib, self._C_STEP)(C.byref(self.p), *self._args, self._actions(actions).data_ptr(), *after_actions,
                                                C.byref(self._out), self.seed, self.step_count, self._stream()), self._C_STEP)
        self.step_count += 1
        return self.obs, self.reward, self.terminated, self.truncated

    def rollout(self, actions: torch.Tensor, obs_out=None, rew_out=None, term_out=None, trunc_out=None, dones_out=None,
                persistent: bool = False):
        """K fused steps with pre-staged actions [K, n, 2]; optional [K, ...] output storage (else the batch's own rows,
        overwritten).  persistent=True runs them as ONE launch with the state in registers (_C_PERSISTENT: quad form,
        n <= 32 768; the elevation scan / the visual camera of step k overlapped with step k + 1); same results."""
        self._rollout(actions, (obs_out, rew_out, term_out, trunc_out, dones_out), persistent)

    def _rollout(self, actions, rows, persistent):
        K = actions.shape[0]
        assert actions.shape == (K, self.n, 2) and actions.dtype == torch.float32 and actions.is_contiguous()
        if not persistent:
            return self._launch_rollout(self._C_ROLLOUT, actions, rows)
        assert rows[0] is not None or K == 1 or not self._PERSISTENT_NEEDS_ROWS, "a persistent rollout needs per-step output rows"
        segments = self._ring_segments(K)
        if len(segments) == 1:
            return self._launch_rollout(self._C_PERSISTENT, actions, rows)
        for k0, k in segments:
            self._launch_rollout(self._C_PERSISTENT, actions[k0:k0 + k], [None if t is None else t[k0:k0 + k] for t in rows])

    def _launch_rollout(self, fn, actions, rows):
        obs_out, rew_out, term_out, trunc_out, dones_out = rows
        if obs_out is not None:
            key = (obs_out.data_ptr(), rew_out.data_ptr(), term_out.data_ptr(), trunc_out.data_ptr(),
                   None if dones_out is None else dones_out.data_ptr())
            if self._out_key != key:      # the struct of the caller's storage rows, rebuilt when they change
                self._out_key, self._out_rows = key, A.WlStepOut(*key)
            out, os_, vs_ = self._out_rows, self.n * self.OBS_DIM, self.n
        else:
            out, os_, vs_ = self._out, 0, 0
        K = actions.shape[0]
        A.check(getattr(self.lib, fn)(C.byref(self.p), *self._args, actions.data_ptr(), C.byref(out), os_, vs_, K, self.seed,
                                      self.step_count, self._stream()), fn)
        self.step_count += K

    def _ring_segments(self, n_steps: int):
        """the launches (first step, steps) of a persistent run of n_steps steps from step_count (ring_plan), after clearing the
        ring slots they fold away; warns once per batch when the run is split"""
        segments, zero = ring_plan(self.step_count, n_steps, self.metrics_slots)
        if len(segments) > 1 and not self._ring_split_warned:
            import warnings
            warnings.warn(f"a persistent rollout of {n_steps} steps with a metric ring of {self.metrics_slots} slots is run as 1 + "
                          f"{n_steps - 1} steps: the ring then misses the first step's episode counts (choose a rollout length that is "
                          "not a multiple of metrics_slots to keep them)", stacklevel=4)
            self._ring_split_warned = True
        if zero:
            self.metrics_raw[zero] = 0
        return segments


class DriftBatch(_EnvBatch):
    """n drift envs resident on one GPU (csrc/wl_drift.hip)."""

    OBS_DIM = 14
    LANES = (0, 1, 2, 4)           # 2: lane form with the scalar wheel loop (drift only)
    _C_RESET, _C_STEP, _C_ROLLOUT, _C_PERSISTENT = "wl_drift_reset", "wl_drift_step", "wl_drift_rollout", "wl_drift_rollout_persistent"
    _PERSISTENT_NEEDS_ROWS = False

    def __init__(self, n_envs: int, device="cuda:0", params: A.WlDriftParams | None = None, seed: int = 42,
                 env_offset: int = 0, randomize: bool = True, metrics_slots: int = 1, startup=None):
        p = params if params is not None else drift_params()
        # reference poses are drawn ONCE at construction (events.py:31,35)
        ref_table = torch.zeros(3, 32, dtype=torch.float32)
        tr = (startup.track_radius, startup.track_straight) if startup is not None else (0.8, 0.8)
        g = torch.Generator().manual_seed(int(seed))
        ref_table[:, : p.num_ref_points] = stadium_reference_poses(torch.rand(p.num_ref_points, generator=g), *tr)
        super().__init__(n_envs, device, p, seed, env_offset, metrics_slots, ref_table)
        self._startup_events(randomize, startup)

    # startup events (mushr_drift_env_cfg.py:98-119, 145-154)
    def _startup_events(self, randomize: bool, su=None):
        if su is None:  # the RSS drift defaults
            from .envs.flatten import StartupSpec
            su = StartupSpec(wheel_mu_s=(0.3, 0.5), wheel_mu_d=(0.3, 0.5), mu_buckets=20, mu_consistent=True,
                             damping=(10.0, 50.0), mass_add=(0.3, 0.5))
        apply_startup_events(self.lib, self._bufs, su, self.seed, self._stream(), randomize)

    def observe(self, noise: torch.Tensor | None = None) -> torch.Tensor:
        A.check(self.lib.wl_drift_observe(C.byref(self.p), C.byref(self._bufs),
                                          None if noise is None else noise.data_ptr(), self.obs.data_ptr(), self.seed,
                                          self.step_count, self._stream()), "wl_drift_observe")
        return self.obs

    def step(self, actions: torch.Tensor, noise: torch.Tensor | None = None):
        """actions [n,2] fp32 on device -> (obs [n,14], reward [n], terminated u8 [n], truncated u8 [n]) (views)"""
        return self._step(actions, None if noise is None else noise.data_ptr())

    def rollout(self, actions: torch.Tensor, obs_out: torch.Tensor | None = None, rew_out: torch.Tensor | None = None,
                term_out: torch.Tensor | None = None, trunc_out: torch.Tensor | None = None, persistent: bool = False,
                dones_out: torch.Tensor | None = None):
        """K fused steps with pre-staged actions [K,n,2]; optional [K,...] output storage (else overwrite).
        persistent=True runs them as ONE launch with the state held in registers (wl_drift_rollout_persistent)."""
        self._rollout(actions, (obs_out, rew_out, term_out, trunc_out, dones_out), persistent)

    def rollout_policy(self, actor_critic, storage, evaluate_critic: bool = True, start: int = 0, count: int | None = None):
        """The runner's collection loop (modified_rsl_rl_runner.py:70-80) as one launch: `count` times
        { actor(obs) on the matrix pipe -> sample -> env.step } with the env state and the observation in registers
        (wl_drift_rollout_policy), filling storage rows start .. start + count; then (optionally) the critic over ALL
        observation rows of the storage in one wl_mlp_forward.  Row `start` of storage.observations is seeded with the
        current observation; self.obs ends as the last one."""
        K = storage.n_steps - start if count is None else int(count)
        assert storage.n_envs == self.n and actor_critic.actor.in_dim == self.OBS_DIM and 0 <= start and start + K <= storage.n_steps
        for k0, k in self._ring_segments(K):
            s = start + k0
            storage.observations[s].copy_(self.obs)
            actor, io = actor_critic.actor.struct(), storage.struct(s)
            A.check(self.lib.wl_drift_rollout_policy(C.byref(self.p), C.byref(self._bufs), C.byref(actor),
                                                     actor_critic.std.data_ptr(), C.byref(io), k, self.seed, self.step_count,
                                                     self._stream()), "wl_drift_rollout_policy")
            self.step_count += k
            if k > 0:
                e = s + k
                self.obs.copy_(storage.observations[e])
                self.reward.copy_(storage.rewards[e - 1])
                self.terminated.copy_(storage.terminated[e - 1])
                self.truncated.copy_(storage.time_outs[e - 1])
                self.dones.copy_(storage.dones[e - 1])
        if evaluate_critic:
            storage.values.copy_(actor_critic.critic(storage.observations).squeeze(-1))
        return storage


class FlatPatches:
    """Level ground found on a field by the device (wl_flat_patches; IsaacLab's TerrainImporter.flat_patches): for each of the
    `tiles` windows (WlPatchTile rows as a structured array: envs.terrain_gen_cfg.patch_table / field_patch_table) `n_patches`
    lattice points whose disc of neighbours is level.  `xy` float32 [T, P, 2], `z` float32 [T, P], `tries` int32 [T, P] (the accepted
    attempt's index, -1: none -- the slot holds its window's centre) live on the device at fixed addresses: the field's refresh() --
    so regenerate() -- finds them again in place.  `raise_on` bool [T]: tiles on which a failed slot is an error (checked after
    every search, one synchronisation); elsewhere `failed` counts them, read lazily.  `name`: the set of a GENERATED field's config
    (find_flat_patches): the windows then follow the field's generator -- when a redraw changes what the table was resolved from (a
    new config; another seed without a curriculum, which moves the sub-terrain types) the table is resolved again from the field's
    config, checked and uploaded into the same device buffer before the search; it must keep its tile and patch counts."""

    def __init__(self, hf: "DeviceHeightField", tiles, n_patches: int, seed: int = 0, stream: int = A.TS_PATCH, raise_on=None, labels=None,
                 name: str | None = None, cfg=None):
        import weakref

        import numpy as np
        self.lib = A.load()
        self.hf, self.device = hf, hf.device
        if self.device.type != "cuda":
            raise A.HipExtensionMissing("flat patches are found on a HIP device (device='cuda:N'); there is no CPU path")
        table = np.ascontiguousarray(tiles)
        if table.dtype.itemsize != C.sizeof(A.WlPatchTile) or table.ndim != 1 or not len(table):
            raise ValueError("flat patches: `tiles` is a non-empty 1-d array of WlPatchTile rows (terrain_gen_cfg.PATCH_DTYPE)")
        self.n_tiles, self.n_patches, self.seed = len(table), int(n_patches), int(seed) & (2 ** 64 - 1)
        self.params = A.WlFlatPatchParams(self.n_tiles, self.n_patches, int(stream), 0, self.seed)
        self.name, self._cfg = name, cfg
        self._resolved_from = self._table_key(hf.generator) if name is not None else None
        self.tiles = torch.zeros(self.n_tiles * C.sizeof(A.WlPatchTile), dtype=torch.uint8, device=self.device)
        self._searched = torch.zeros(self.n_tiles, dtype=torch.bool, device=self.device)
        self._set_table(table, raise_on, labels)
        self.xy = torch.zeros(self.n_tiles, self.n_patches, 2, dtype=torch.float32, device=self.device)
        self.z = torch.zeros(self.n_tiles, self.n_patches, dtype=torch.float32, device=self.device)
        self.tries = torch.full((self.n_tiles, self.n_patches), -1, dtype=torch.int32, device=self.device)
        hf._shared["patches"].append(weakref.ref(self))
        self.find()

    @staticmethod
    def _table_key(cfg, sampling: bool = True):
        """what a generator config's patch table depends on: every field but the seed -- and the seed too without a curriculum (it
        then draws every tile's sub-terrain type); sampling=False: without the generator-level flat_patch_sampling"""
        if cfg is None:
            return None
        fields = dict(vars(cfg))
        seed = fields.pop("seed", None)
        if not sampling:
            fields.pop("flat_patch_sampling", None)
        return repr(fields), (None if cfg.curriculum else seed)

    def _set_table(self, table, raise_on, labels):
        """validate a table on the host and put it into the device buffer the kernel reads, in place"""
        import numpy as np
        table = np.ascontiguousarray(table)
        rc = self.lib.wl_flat_patch_check(C.byref(self.hf.struct), C.byref(self.params), table.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise ValueError(f"flat patches: {self.n_tiles} windows x {self.n_patches} patches are outside the finder's range on a field of "
                             f"{self.hf.struct.nx} x {self.hf.struct.ny} points ({A.ERRORS.get(rc, rc)}; include/wheeledlab_amd_terrain.h: non-empty "
                             f"windows, discs inside the lattice, radius <= {A.PATCH_MAX_RADIUS} cells, max_tries <= {A.PATCH_MAX_TRIES})")
        self.table = table
        self.raise_on = np.zeros(self.n_tiles, bool) if raise_on is None else np.asarray(raise_on, bool).reshape(self.n_tiles)
        self.labels = list(labels) if labels is not None else [f"tile {t}" for t in range(self.n_tiles)]
        self.tiles.copy_(torch.from_numpy(table.view(np.uint8).reshape(-1).copy()))
        self._searched.copy_(torch.from_numpy(table["max_tries"] > 0))

    def _follow_generator(self):
        """resolve the table again when the field's generator config no longer is what it was resolved from: from the field's
        config when that carries the set, else from the config the set was made with, moved to the field's seed"""
        gen = self.hf.generator
        if self.name is None or gen is None:
            return
        key = self._table_key(gen)
        if key == self._resolved_from:
            return
        from .envs import terrain_gen_cfg as G
        src = gen
        if self.name not in G.patch_names(gen):
            src = self._cfg.replace(seed=gen.seed)
            if self._table_key(src, sampling=False) != self._table_key(gen, sampling=False):
                raise ValueError(f"flat patches '{self.name}': the field was redrawn from a generator config that neither carries the "
                                 "sampling nor equals, but for the seed, the one the patches were resolved from: put flat_patch_sampling "
                                 "into the config handed to regenerate()")
        table, n_patches, raise_on, labels = G.patch_table(src, self.name)
        if len(table) != self.n_tiles or n_patches != self.n_patches:
            raise ValueError(f"flat patches '{self.name}': the new generator config gives {len(table)} tiles x {n_patches} patches, the set "
                             f"holds {self.n_tiles} x {self.n_patches} at fixed addresses -- build a new field and new patches instead")
        self._set_table(table, raise_on, labels)
        self._resolved_from = key

    def find(self):
        """search the field's codes as they are now, on the current stream, into the same buffers"""
        self._follow_generator()
        A.check(self.lib.wl_flat_patches(C.byref(self.hf.struct), C.byref(self.params), self.tiles.data_ptr(), self.xy.data_ptr(),
                                         self.z.data_ptr(), self.tries.data_ptr(), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                "wl_flat_patches")
        if self.raise_on.any():
            bad = ((self.tries < 0).any(1).cpu().numpy()) & self.raise_on
            if bad.any():
                t = int(bad.argmax())
                raise ValueError(f"flat patches: {self.labels[t]} has no level ground for {int((self.tries[t] < 0).sum())} of its "
                                 f"{self.n_patches} patches within {int(self.table['max_tries'][t])} tries (radius {int(self.table['radius_cells'][t])} "
                                 f"cells, height difference {int(self.table['max_diff_codes'][t])} codes): relax the sampling or set on_failure='centre'")
        return self

    @property
    def failed(self) -> int:
        """slots of the searched tiles (max_tries > 0) that found nothing and hold their window's centre (one synchronisation)"""
        return int(((self.tries < 0) & self._searched[:, None]).sum())

    def positions(self) -> torch.Tensor:
        """[T, P, 3]: (x, y, z) of every patch"""
        return torch.cat([self.xy, self.z[..., None]], -1)


def find_flat_patches(hf: DeviceHeightField, cfg, seed: int = 0, name: str = "init_pos", stream: int = A.TS_PATCH) -> FlatPatches:
    """Flat patches on any field: `cfg` a FlatPatchSamplingCfg (or its fields as a dict) -- one window, the field itself -- or the
    TerrainGeneratorCfg the field was generated from -- one window per tile, the patches it and its sub-terrains call `name`."""
    from .envs import terrain_gen_cfg as G
    if isinstance(cfg, G.TerrainGeneratorCfg):
        geo = G.lattice(cfg)
        if (geo["nx"], geo["ny"]) != (hf.struct.nx, hf.struct.ny):
            raise ValueError(f"flat patches: the generator config gives {geo['nx']} x {geo['ny']} points, the field has {hf.struct.nx} x {hf.struct.ny}")
        if hf.generator is not None and FlatPatches._table_key(hf.generator, False) != FlatPatches._table_key(cfg.replace(seed=hf.generator.seed), False):
            raise ValueError("flat patches: `cfg` lays its tiles out otherwise than the generator config the field was last drawn from "
                             "(they may differ in the seed and in the generator-level flat_patch_sampling alone)")
        cfg = cfg.replace(seed=hf.generator.seed) if hf.generator is not None else cfg
        table, P, raise_on, labels = G.patch_table(cfg, name)
    else:
        table, P, raise_on, labels = G.field_patch_table(cfg, hf.struct.nx, hf.struct.ny, hf.x0, hf.y0, hf.cell, hf.z_scale)
    return FlatPatches(hf, table, P, seed, stream, raise_on, labels, *((name, cfg) if isinstance(cfg, G.TerrainGeneratorCfg) else ()))


class TerrainLevels:
    """The terrain curriculum's device tables (WlTerrainLevels): `level` / `type` int32 [n] -- the row and column of every env's
    tile, LIVE: the step kernels move `level` at episode ends -- and `origins` float32 [rows * cols, 2], the tile centres.  Built
    from the TerrainGeneratorCfg of a generated field for envs env_offset .. env_offset + n of a world of `world_envs` envs (a
    shard holds its slice of the one big batch's assignment: envs.terrain_levels.initial_assignment), or from ready tables
    (from_tables).  Hand it to ElevBatch(terrain_levels=...).

    With `flat_patches` (a FlatPatches of rows * cols tiles, P patches each) every patch is a VIRTUAL COLUMN: the tables the kernels
    read have cols * P columns, `origins` IS the finder's xy buffer ([tile][k][2] = row-major [rows][cols * P][2]: found again in
    place when the field is redrawn) and type[e] = column * P + slot, dealt on the device (wl_flat_patch_deal; redeal(epoch) deals
    again).  The step kernels, unchanged, then spawn about a patch and move levels as before.  `tile_cols`, `tile_origins` and
    `terrain_types` stay the real grid's."""

    n_patches, patches, grid = 1, None, None

    def __init__(self, cfg, n_envs: int, device="cuda:0", env_offset: int = 0, world_envs: int | None = None,
                 max_init_terrain_level: int | None = None, seed: int = 42, flat_patches: "FlatPatches | None" = None):
        from .envs import terrain_levels as TL
        level, types = TL.initial_assignment(cfg, n_envs, env_offset, world_envs, max_init_terrain_level, seed)
        if flat_patches is None:
            self._set(level, types, TL.tile_origins(cfg), int(cfg.num_rows), int(cfg.num_cols), device)
        else:
            self._set_patches(level, flat_patches, TL.tile_origins(cfg), int(cfg.num_rows), int(cfg.num_cols), device, env_offset, world_envs, seed)
        self.max_init_terrain_level = TL.clamp_max_init(cfg, max_init_terrain_level)

    @classmethod
    def on_patches(cls, flat_patches: "FlatPatches", n_envs: int, rows: int = 1, cols: int = 1, level=None, tile_origins=None,
                   device="cuda:0", env_offset: int = 0, world_envs: int | None = None, seed: int = 42, grid=None):
        """levels over a FlatPatches of rows * cols tiles without a generator config; the default is the one-row table of a field
        that was not generated (a height array, a rasterised mesh): one tile, level 0 for good (the wrap rule keeps it there).  A
        generated grid WITHOUT a curriculum is one row too -- rows = 1, cols = every tile, `grid` = (its rows, its columns): the
        envs are spread over all tiles and stay where they are."""
        import numpy as np
        self = cls.__new__(cls)
        self.grid = None if grid is None else (int(grid[0]), int(grid[1]))
        o = np.zeros((int(rows) * int(cols), 2), np.float32) if tile_origins is None else tile_origins
        self._set_patches(np.zeros(int(n_envs), np.int32) if level is None else level, flat_patches, o, rows, cols, device, env_offset,
                          world_envs, seed)
        self.max_init_terrain_level = int(rows) - 1
        return self

    def _set_patches(self, level, fp, tile_origins, rows, cols, device, env_offset, world_envs, seed):
        n = len(level)
        self.env_offset, self.world_envs, self.seed = int(env_offset), int(n if world_envs is None else world_envs), int(seed) & (2 ** 64 - 1)
        if fp.n_tiles != int(rows) * int(cols) or fp.device != _canonical_device(device):
            raise ValueError(f"flat patches of {fp.n_tiles} tiles on {fp.device} for {rows} x {cols} tiles on {_canonical_device(device)}")
        self.patches, self.n_patches = fp, fp.n_patches
        types = torch.zeros(n, dtype=torch.int32, device=fp.device)
        self._set(level, types, fp.xy.view(-1, 2), int(rows), int(cols) * fp.n_patches, device, share_origins=True)
        self.tile_cols = int(cols)
        self.tile_origins = torch.as_tensor(tile_origins).to(self.device, torch.float32).reshape(-1, 2).contiguous().clone()
        self.redeal(0)

    def redeal(self, epoch: int):
        """deal every env a slot of its column again (wl_flat_patch_deal on the current stream: no host work, no synchronisation);
        the slot counts from the env's next reset on.  Without flat patches: nothing to deal."""
        if self.patches is None:
            return
        lib = A.load()
        A.check(lib.wl_flat_patch_deal(self.type.shape[0], self.env_offset, self.world_envs, self.tile_cols, self.n_patches, int(epoch),
                                       self.seed, self.type.data_ptr(), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                "wl_flat_patch_deal")

    @property
    def terrain_types(self) -> torch.Tensor:
        """[n] int32: the column of every env's tile on the real grid (type // P; `type` itself without flat patches)"""
        if self.patches is None:
            return self.type
        col = torch.div(self.type, self.n_patches, rounding_mode="floor")
        return col if self.grid is None else col % self.grid[1]

    @property
    def terrain_levels(self) -> torch.Tensor:
        """[n] int32: the row of every env's tile on the real grid -- `level` itself (LIVE) unless a grid without a curriculum
        was laid out as one row"""
        return self.level if self.grid is None else torch.div(torch.div(self.type, self.n_patches, rounding_mode="floor"), self.grid[1],
                                                               rounding_mode="floor")

    @property
    def grid_shape(self) -> tuple:
        return (self.rows, self.tile_cols) if self.grid is None else self.grid

    @classmethod
    def from_tables(cls, level, types, origins, rows: int, cols: int, device="cuda:0"):
        """level / types [n] integers in [0, rows) / [0, cols), origins [rows * cols, 2] metres"""
        self = cls.__new__(cls)
        self._set(level, types, origins, rows, cols, device)
        self.max_init_terrain_level = int(rows) - 1
        return self

    def _set(self, level, types, origins, rows, cols, device, share_origins: bool = False):
        self.device, self.rows, self.cols = _canonical_device(device), int(rows), int(cols)
        self.level = torch.as_tensor(level).to(self.device, torch.int32).contiguous().clone()
        self.type = torch.as_tensor(types).to(self.device, torch.int32).contiguous().clone()
        # (shared: the finder's own buffer, which it fills again in place)
        self.origins = origins if share_origins else torch.as_tensor(origins).to(self.device, torch.float32).reshape(-1, 2).contiguous().clone()
        self.tile_cols, self.tile_origins = self.cols, self.origins
        if self.rows < 1 or self.cols < 1 or self.origins.shape[0] != self.rows * self.cols or self.level.shape != self.type.shape or self.level.dim() != 1:
            raise ValueError(f"terrain levels: {self.rows} x {self.cols} tiles need origins [{self.rows * self.cols}, 2] and level / type of one length")
        if self.level.numel() and (int(self.level.min()) < 0 or int(self.level.max()) >= self.rows or int(self.type.min()) < 0
                                   or int(self.type.max()) >= self.cols):
            raise ValueError(f"terrain levels outside [0, {self.rows}) or types outside [0, {self.cols})")
        self.struct = A.WlTerrainLevels(self.level.data_ptr(), self.type.data_ptr(), self.origins.data_ptr(), self.rows, self.cols)

    def env_origins_xy(self) -> torch.Tensor:
        """[n, 2]: the centre of every env's tile as the levels stand"""
        return self.origins[self.level.long() * self.cols + self.type.long()]

    def mean_level(self) -> torch.Tensor:
        """0-dim device tensor: what the terrain_levels curriculum term reports"""
        return self.level.float().mean()


class ElevBatch(_EnvBatch):
    """n elevation-task envs on one GPU (same SoA state matrix; rows WL_S_CMD_* carry the goal command)."""

    OBS_DIM = A.ELEV_OBS_DIM
    _C_RESET, _C_STEP, _C_ROLLOUT, _C_PERSISTENT = "wl_elev_reset", "wl_elev_step", "wl_elev_rollout", "wl_elev_rollout_persistent"

    def __init__(self, n_envs: int, device="cuda:0", params: A.WlElevParams | None = None, seed: int = 42,
                 env_offset: int = 0, heightfield=None, metrics_slots: int = 1, startup=None, terrain_levels: TerrainLevels | None = None):
        from .params import elev_params
        from .terrain import synthetic_heightfield
        super().__init__(n_envs, device, params if params is not None else elev_params(), seed, env_offset, metrics_slots)
        self.set_terrain_levels(terrain_levels)
        self.hf = DeviceHeightField(heightfield if heightfield is not None else synthetic_heightfield(), self.device)
        self.height, self._hf = self.hf.heights, self.hf.struct       # the DECODED fp32 grid (what the kernels see); the ABI struct
        self._args = (C.byref(self._bufs), C.byref(self._hf))
        # startup events (elevation cfg :387-407): wheel friction fixed (2.0, 1.0), base mass += U(0.2, 0.5)
        if startup is None:
            from .envs.flatten import StartupSpec
            startup = StartupSpec(wheel_mu_s=(2.0, 2.0), wheel_mu_d=(1.0, 1.0), mu_buckets=5, mu_consistent=False,
                                  damping=(1000.0, 1000.0), mass_add=(0.2, 0.5))
        apply_startup_events(self.lib, self._bufs, startup, self.seed, self._stream())

    def set_terrain_levels(self, levels: TerrainLevels | None):
        """switch the terrain curriculum on (a TerrainLevels of this batch's envs, on its device) or off (None): the batch's
        params carry the tables from here on (WlElevParams.levels; the struct is this batch's own copy when it changes)"""
        if levels is not None and (levels.level.shape[0] != self.n or levels.device != _canonical_device(self.device)):
            raise ValueError(f"terrain levels of {levels.level.shape[0]} envs on {levels.device} for a batch of {self.n} on {self.device}")
        if levels is not None or self.p.levels.level:
            q = type(self.p)()
            C.pointer(q)[0] = self.p            # a copy: a params struct shared with other batches keeps its own tables
            q.levels = levels.struct if levels is not None else A.WlTerrainLevels()
            self.p = q
        self.levels = levels

    def observe(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """observation of the current state into self.obs (or a caller's [n, 689] buffer)"""
        out = self.obs if out is None else out
        A.check(self.lib.wl_elev_observe(C.byref(self.p), C.byref(self._bufs), C.byref(self._hf), out.data_ptr(),
                                         self._stream()), "wl_elev_observe")
        return out

    def collect_rollout(self, actor_critic, storage, start: int = 0, count: int | None = None, deterministic: bool = False):
        """rows start .. start + count - 1 of the storage (and observation row start + count) from observation row `start`: the
        runner's whole collection loop as ONE launch (wl_elev_collect_rollout: the actor's first layer in the blocks' registers,
        their observation rows in LDS, the critic beside the physics).  Quad form only (n <= 32 768)."""
        st = storage
        count = st.n_steps - start if count is None else int(count)
        for k0, k in self._ring_segments(count):
            key = (st.observations.data_ptr(), actor_critic.actor.w1.data_ptr(), actor_critic.critic.w1.data_ptr(), actor_critic.std.data_ptr())
            if getattr(self, "_collect_key", None) != key:
                assert st.n_envs == self.n and st.observations.shape[2] == self.OBS_DIM and st.observations.is_contiguous()
                self._collect_key = key
                self._collect_nets = (actor_critic.actor.struct(), actor_critic.critic.struct())
            a, c = self._collect_nets
            obs, s = st.observations, int(start) + k0
            io = A.WlCollectIo(obs[s].data_ptr(), st.actions[s].data_ptr(), st.mu[s].data_ptr(), st.actions_log_prob[s].data_ptr(),
                               st.values[s].data_ptr())
            out = A.WlStepOut(obs[s + 1].data_ptr(), st.rewards[s].data_ptr(), st.terminated[s].data_ptr(), st.time_outs[s].data_ptr(),
                              st.dones[s].data_ptr())
            A.check(self.lib.wl_elev_collect_rollout(C.byref(self.p), C.byref(self._bufs), C.byref(self._hf), C.byref(a), C.byref(c),
                                                     actor_critic.std.data_ptr(), C.byref(io), C.byref(out), k, int(bool(deterministic)),
                                                     self.seed, self.step_count, self._stream()), "wl_elev_collect_rollout")
            self.step_count += k


class VisualBatch(_EnvBatch):
    """n visual-task envs on one GPU: flat black/white traversability plane + ray-cast grey camera."""

    OBS_DIM = A.VIS_OBS_DIM
    _C_RESET, _C_STEP, _C_ROLLOUT, _C_PERSISTENT = "wl_visual_reset", "wl_visual_step", "wl_visual_rollout", "wl_visual_rollout_persistent"

    def __init__(self, n_envs: int, device="cuda:0", params=None, seed: int = 42, env_offset: int = 0, trav_map=None,
                 spacing=(0.5, 0.5), metrics_slots: int = 1, startup=None, map_kwargs=None):
        import numpy as np

        from .params import visual_params
        from .travmap import generate_traversability_map, spawn_cells
        super().__init__(n_envs, device, params if params is not None else visual_params(), seed, env_offset, metrics_slots)
        dev = self.device
        if trav_map is None:  # generated at construction from a seeded RNG (the reference uses the global numpy RNG)
            trav_map = generate_traversability_map(rng=np.random.RandomState(self.seed), **(map_kwargs or {}))
        trav_map = np.ascontiguousarray(np.asarray(trav_map, dtype=bool))
        if trav_map.ndim != 2 or trav_map.shape[0] != trav_map.shape[1]:
            # map[y_idx, x_idx] with x clamped to rows - 1 and y to cols - 1 (traversability_utils.py:78-88) only stays inside a
            # square map: the reference raises IndexError past the shorter side, and the kernels refuse such a map
            raise ValueError(f"VisualBatch: the traversability map must be square, got {trav_map.shape}")
        self.trav_map = torch.from_numpy(trav_map.astype(np.uint8)).to(dev)
        self.cells = torch.from_numpy(spawn_cells(trav_map)).contiguous().to(dev)
        # one bit per cell (bit k & 31 of word k >> 5, k = iy * cols + ix): what the camera kernels keep in LDS
        bits = np.packbits(np.concatenate([trav_map.reshape(-1), np.zeros((-trav_map.size) % 32, bool)]), bitorder="little")
        self.trav_bits = torch.from_numpy(bits.view(np.int32).copy()).to(dev)
        self._map = A.WlTravMap(self.trav_map.data_ptr(), self.cells.data_ptr(), trav_map.shape[0], trav_map.shape[1],
                                self.cells.shape[0], float(spacing[0]), float(spacing[1]), self.trav_bits.data_ptr())
        self._args = (C.byref(self._bufs), C.byref(self._map))
        if startup is None:
            from .envs.flatten import StartupSpec
            startup = StartupSpec(wheel_mu_s=(0.5, 0.5), wheel_mu_d=(0.5, 0.5), damping=(1000.0, 1000.0), mass_add=(0.0, 0.0))
        apply_startup_events(self.lib, self._bufs, startup, self.seed, self._stream())

    def sample_augmentation(self, generator: torch.Generator | None = None):
        """one (brightness, contrast, blur sigma) per call, like torchvision's ColorJitter(brightness=.8, contrast=.2)
        and GaussianBlur(5, sigma=(0.1, 5)) on a batched tensor (mdp_sensors/observations.py:21-23)"""
        # ColorJitter.forward: fn_idx = torch.randperm(4) over (brightness, contrast, saturation, hue), then the factors; ONE
        # draw per call, i.e. per batch (the reference passes the whole [B, C, H, W] tensor).  Hue / saturation: see the header.
        order = torch.randperm(4, generator=generator).tolist()
        u = torch.rand(3, generator=generator)
        self.p.brightness = float(0.2 + 1.6 * u[0])
        self.p.contrast = float(0.8 + 0.4 * u[1])
        self.p.blur_sigma = float(0.1 + 4.9 * u[2])
        self.p.contrast_first = int(order.index(1) < order.index(0))

    def observe(self) -> torch.Tensor:
        A.check(self.lib.wl_visual_observe(C.byref(self.p), C.byref(self._bufs), C.byref(self._map), self.obs.data_ptr(),
                                           self._stream()), "wl_visual_observe")
        return self.obs

    def depth(self, heightfield, max_depth: float = 20.0, out: torch.Tensor | None = None) -> torch.Tensor:
        """distance_to_image_plane of the camera against a heightfield -> [n, 60, 80] (BASELINE config 5); `heightfield` is
        (height [ny, nx], x0, y0, cell) or a DepthCamera (build it once when rendering every step)"""
        cam = heightfield if isinstance(heightfield, DepthCamera) else _cached_depth_camera(self, heightfield)
        return cam.render(self, max_depth, out)


class VisualDepthBatch(VisualBatch):
    """n envs of the visual-DEPTH extension task (BASELINE.json configs[4]; not a reference id): the visual task's step driven on a
    heightfield terrain with the camera's 60 x 80 depth image as the observation -- obs [n, 4808] = distance_to_image_plane |
    base_lin_vel | base_ang_vel | last_action.  Two launches per env.step(): the step (wl_visual_step_hf: lane or quad of lanes
    = env, HeightFieldGround contacts) and the depth ray-cast (wl_visual_depth_rows).  `heightfield`: (height [ny, nx], x0, y0,
    cell), default the synthetic 800 x 800 terrain; the traversability map should cover it (default: an 80 x 80 map of 0.5 m
    cells = the terrain's 40 m square, generated like the reference's from the seed)."""

    OBS_DIM = A.VISDEPTH_OBS_DIM
    _C_RESET = "wl_visual_reset_hf"

    def __init__(self, n_envs: int, device="cuda:0", params=None, seed: int = 42, env_offset: int = 0, trav_map=None,
                 spacing=(0.5, 0.5), metrics_slots: int = 1, startup=None, map_kwargs=None, heightfield=None, max_depth: float = 20.0):
        from .terrain import synthetic_heightfield
        if trav_map is None and map_kwargs is None:
            map_kwargs = dict(map_size=(80, 80), env_size=(40, 40), sub_group_size=(20, 20), num_walkers=1)
        super().__init__(n_envs, device, params, seed, env_offset, trav_map, spacing, metrics_slots, startup, map_kwargs)
        self.hf = DeviceHeightField(heightfield if heightfield is not None else synthetic_heightfield(), self.device)
        self.height = self.hf.heights
        self.max_depth = float(max_depth)
        self.camera = DepthCamera(self.hf, self.device, self.p)
        self._hf, self._pyr = self.camera._hf, self.camera._pyr
        self._args = (C.byref(self._bufs), C.byref(self._map), C.byref(self._hf))

    def observe(self, out: torch.Tensor | None = None) -> torch.Tensor:
        out = self.obs if out is None else out
        A.check(self.lib.wl_visual_depth_observe(C.byref(self.p), C.byref(self._bufs), C.byref(self._hf), self._pyr,
                                                 self.max_depth, out.data_ptr(), self._stream()), "wl_visual_depth_observe")
        return out

    def sample_augmentation(self, generator=None):
        """the depth image is not augmented (mdp_sensors/observations.py:93-95 returns the raw distances)"""

    def step(self, actions: torch.Tensor):
        self._step_into(self._actions(actions).data_ptr(), self._out)
        return self.obs, self.reward, self.terminated, self.truncated

    def _step_into(self, actions_ptr, out):
        A.check(self.lib.wl_visual_depth_step(C.byref(self.p), *self._args, self._pyr, self.max_depth, actions_ptr,
                                              C.byref(out), self.seed, self.step_count, self._stream()), "wl_visual_depth_step")
        self.step_count += 1

    def rollout(self, actions: torch.Tensor, obs_out=None, rew_out=None, term_out=None, trunc_out=None, dones_out=None,
                persistent: bool = False):
        """K steps with pre-staged actions [K, n, 2]; optional [K, ...] output storage (else overwritten in place)"""
        K = actions.shape[0]
        assert actions.shape == (K, self.n, 2) and actions.dtype == torch.float32 and actions.is_contiguous() and not persistent
        for k in range(K):
            out = self._out if obs_out is None else A.WlStepOut(obs_out[k].data_ptr(), rew_out[k].data_ptr(), term_out[k].data_ptr(),
                                                                trunc_out[k].data_ptr(), None if dones_out is None else dones_out[k].data_ptr())
            self._step_into(actions[k].data_ptr(), out)

    def depth(self, heightfield=None, max_depth: float | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """the task's own terrain unless another heightfield is given"""
        if heightfield is None:
            return self.camera.render(self, self.max_depth if max_depth is None else max_depth, out)
        return super().depth(heightfield, 20.0 if max_depth is None else max_depth, out)


class DepthCamera:
    """The visual task's pinhole camera rendering distance_to_image_plane against a heightfield (wl_visual_depth): its parameters
    and a view of the field (`hf`: its own outside plane, the field's buffers and its one bound pyramid), renders the poses of ANY
    batch (rows WL_S_PX.. / WL_S_QW.. of its state matrix).  Reference hook: mdp_sensors/observations.py:89-95; camera
    visual/mushr_visual_env_cfg.py:230-246."""

    IMG_H, IMG_W = 60, 80

    def __init__(self, heightfield, device="cuda:0", params: A.WlVisualParams | None = None, outside_z: float | None = None):
        from .params import visual_params
        self.lib = A.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise A.HipExtensionMissing("DepthCamera needs a HIP device; there is no CPU path")
        self.p = params if params is not None else visual_params()
        self.hf = DeviceHeightField(heightfield, self.device, outside_z)     # a tuple (quantised here) or a batch's own `.hf` (shared)
        self.height, self._hf = self.hf.heights, self.hf.struct
        self._pyr = self.hf.pyramid.data_ptr()    # resolved once: the field rebuilds its pyramid in place (refresh), never moves it

    _stream = _EnvBatch._stream
    pyramid = property(lambda self: self.hf.pyramid)

    def build_pyramid(self):
        """the field's derived tables (the pyramid among them) from its codes as they are now"""
        self.hf.refresh()

    def render(self, batch, max_depth: float = 20.0, out: torch.Tensor | None = None) -> torch.Tensor:
        if out is None:
            out = torch.empty(batch.n, self.IMG_H, self.IMG_W, dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == batch.n * self.IMG_H * self.IMG_W
        A.check(self.lib.wl_visual_depth(C.byref(self.p), C.byref(batch._bufs), C.byref(self._hf), self._pyr,
                                         float(max_depth), out.data_ptr(), self._stream()), "wl_visual_depth")
        return out


class LidarScanner:
    """A lidar (envs.sensors_cfg.LidarCfg) scanning the terrain from the poses of ANY batch (wl_lidar_scan): owns the beam table
    (unit vectors in the sensor frame, built once from the pattern) and the launch parameters.  The terrain is the depth camera's:
    field and pyramid come from the batch's cached DepthCamera, i.e. from the batch's DeviceHeightField (which owns the one pyramid).
    render() -> ranges [n, B], the raw scan: the hit's Euclidean range clipped at max_range, max_range on a miss, 0 from under
    the terrain (what a miss reads in the scene is LidarData's business)."""

    def __init__(self, cfg=None, device="cuda:0"):
        from .envs.sensors_cfg import LidarCfg
        self.lib = A.load()
        self.device = _canonical_device(device)
        if self.device.type != "cuda":
            raise A.HipExtensionMissing("LidarScanner needs a HIP device; there is no CPU path")
        self.cfg = cfg = cfg if cfg is not None else LidarCfg()
        dirs = cfg.pattern_cfg.directions()
        self.n_beams = int(dirs.shape[0])
        if not 1 <= self.n_beams <= A.LIDAR_MAX_BEAMS:
            raise ValueError(f"a lidar pattern of {self.n_beams} beams (1 .. {A.LIDAR_MAX_BEAMS})")
        self.beam_dirs = torch.as_tensor(dirs, dtype=torch.float32).contiguous().to(self.device)
        self.max_range = float(cfg.max_range)
        if not (math.isfinite(self.max_range) and self.max_range > 0):
            raise ValueError(f"lidar max_range must be positive and finite, got {cfg.max_range}")
        q = [float(v) for v in cfg.offset_rot]
        qn = math.sqrt(sum(v * v for v in q))
        if not (math.isfinite(qn) and qn > 0):
            raise ValueError(f"lidar offset_rot must be a non-zero quaternion, got {cfg.offset_rot}")
        self.params = A.WlLidarParams((C.c_float * 3)(*[float(v) for v in cfg.offset_pos]), (C.c_float * 4)(*[v / qn for v in q]),
                                      self.n_beams, self.max_range, int(bool(cfg.attach_yaw_only)))
        self._plane = None

    _stream = _EnvBatch._stream

    def camera_of(self, batch) -> DepthCamera:
        """the terrain the batch's cars stand on, as CameraData does it: the visual-depth task's own camera, the elevation task's
        heightfield, else the z = 0 plane (a 3 x 3 zero grid: beyond it the outside plane is z = 0 as well)"""
        if getattr(batch, "camera", None) is not None:
            return batch.camera
        if hasattr(batch, "hf"):
            return _cached_depth_camera(batch, batch.hf)
        if self._plane is None:       # one tensor per scanner: the batch's camera cache keys on it
            self._plane = (torch.zeros(3, 3, dtype=torch.float32, device=self.device), -1.0, -1.0, 1.0)
        return _cached_depth_camera(batch, self._plane)

    def render(self, batch, out: torch.Tensor | None = None, camera: DepthCamera | None = None) -> torch.Tensor:
        """ranges [batch.n, B] of the batch's current poses; `camera`: another terrain (a DepthCamera) than the batch's own"""
        cam = camera if camera is not None else self.camera_of(batch)
        if out is None:
            out = torch.empty(batch.n, self.n_beams, dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == (batch.n, self.n_beams)
        A.check(self.lib.wl_lidar_scan(C.byref(self.params), C.byref(batch._bufs), C.byref(cam._hf), cam._pyr,
                                       self.beam_dirs.data_ptr(), out.data_ptr(), self._stream()), "wl_lidar_scan")
        return out


def _field_key(heightfield) -> tuple:
    """What tells one `heightfield` argument from another (pure: needs no device).  A DeviceHeightField: its shared buffers' identity and
    the view's outside plane -- it refreshes its tables in place, so no version.  A tuple is a SNAPSHOT: the array object, placement,
    shape, vertical scale (the same codes under another one are another field) and -- for tensors -- the in-place version counter."""
    if isinstance(heightfield, DeviceHeightField):
        return id(heightfield._shared), heightfield.outside_z
    h, x0, y0, cell = heightfield[:4]
    return (id(h), float(x0), float(y0), float(cell), tuple(h.shape), getattr(h, "_version", None),
            float(heightfield[4]) if len(heightfield) > 4 else None)


def _cached_depth_camera(batch, heightfield) -> DepthCamera:
    """one DepthCamera per batch and array (or shared buffers): built on first use, and again when _field_key tells the argument
    from the last one -- a newer snapshot of an array replaces the older (a tuple becomes a DeviceHeightField of its own)"""
    cache = batch.__dict__.setdefault("_depth_cameras", {})
    key = _field_key(heightfield)
    hit = cache.get(key[0])
    if hit is None or hit[0] != key:
        # (the entry holds the argument alive: an id is only unique among live objects)
        hit = cache[key[0]] = (key, heightfield, DepthCamera(heightfield, batch.device, batch.p if isinstance(batch.p, A.WlVisualParams) else None))
    return hit[2]
