"""The device-resident terrain of the heightfield tasks: DeviceHeightField (the codes and every table derived from them), the ways
to make one on the device (generate_heightfield, mesh_heightfield), the level ground found on it (FlatPatches, find_flat_patches),
the curriculum's tables (TerrainLevels) and assemble_terrain, which builds all three for a task from its flattened config -- what
IsaacLab keeps in one TerrainImporter.  Imports neither core (the env batches) nor sensors (the readers of a field).
"""
from __future__ import annotations

import ctypes as C
import math
import weakref

import numpy as np
import torch

from . import _abi as A
from .terrain import default_z_scale, load_obj, synthetic_heightfield


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
        A.check(getattr(A.load(), fn)(C.byref(self.struct), table.data_ptr(), A.stream(self.device)), fn)

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
                                    A.stream(codes.device)), "wl_terrain_generate")


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
                               status.data_ptr(), A.stream(dev)), "wl_mesh_raster")
    words = status.tolist()
    if stats is not None:
        stats.update(zip(("invalid", "binned", "big", "entries"), words))
    bad = words[0]
    if bad:
        raise ValueError(f"{bad} of {f.shape[0]} faces have a vertex index outside [0, {v.shape[0]}) or a non-finite vertex")
    return heights, x0, y0, c32

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
                                         self.z.data_ptr(), self.tries.data_ptr(), A.stream(self.device)),
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

    def __init__(self, cfg, n_envs: int, device="cuda:0", env_offset: int = 0, world_envs: int | None = None,
                 max_init_terrain_level: int | None = None, seed: int = 42, flat_patches: "FlatPatches | None" = None, *, _tables=None):
        if _tables is None:      # (else: on_patches / from_tables, which bring ready tables in place of a config)
            from .envs import terrain_levels as TL
            level, types = TL.initial_assignment(cfg, n_envs, env_offset, world_envs, max_init_terrain_level, seed)
            _tables = (level, types, TL.tile_origins(cfg), cfg.num_rows, cfg.num_cols, TL.clamp_max_init(cfg, max_init_terrain_level), None)
        self._init(*_tables, device, flat_patches, env_offset, world_envs, seed)

    @classmethod
    def on_patches(cls, flat_patches: "FlatPatches", n_envs: int, rows: int = 1, cols: int = 1, level=None, tile_origins=None,
                   device="cuda:0", env_offset: int = 0, world_envs: int | None = None, seed: int = 42, grid=None):
        """levels over a FlatPatches of rows * cols tiles without a generator config; the default is the one-row table of a field
        that was not generated (a height array, a rasterised mesh): one tile, level 0 for good (the wrap rule keeps it there).  A
        generated grid WITHOUT a curriculum is one row too -- rows = 1, cols = every tile, `grid` = (its rows, its columns): the
        envs are spread over all tiles and stay where they are."""
        level = np.zeros(int(n_envs), np.int32) if level is None else level
        o = np.zeros((int(rows) * int(cols), 2), np.float32) if tile_origins is None else tile_origins
        return cls(None, n_envs, device, env_offset, world_envs, None, seed, flat_patches, _tables=(level, None, o, rows, cols, int(rows) - 1, grid))

    @classmethod
    def from_tables(cls, level, types, origins, rows: int, cols: int, device="cuda:0"):
        """level / types [n] integers in [0, rows) / [0, cols), origins [rows * cols, 2] metres"""
        return cls(None, None, device, _tables=(level, types, origins, rows, cols, int(rows) - 1, None))

    def _init(self, level, types, tile_origins, rows, cols, max_init, grid, device, fp, env_offset, world_envs, seed):
        """every attribute of every instance.  `cols` counts the real grid's columns (`tile_cols`); with flat patches `fp` the tables
        get cols * P virtual columns, `types` is dealt on the device and `origins` is the finder's own buffer, which it fills again in place"""
        self.device, self.rows, self.tile_cols = _canonical_device(device), int(rows), int(cols)
        self.grid = None if grid is None else (int(grid[0]), int(grid[1]))
        self.env_offset, self.world_envs, self.seed = int(env_offset), int(len(level) if world_envs is None else world_envs), int(seed) & (2 ** 64 - 1)
        self.max_init_terrain_level = int(max_init)
        self.patches, self.n_patches = fp, 1 if fp is None else fp.n_patches
        if fp is not None:
            if fp.n_tiles != self.rows * self.tile_cols or fp.device != self.device:
                raise ValueError(f"flat patches of {fp.n_tiles} tiles on {fp.device} for {rows} x {cols} tiles on {self.device}")
            types = torch.zeros(len(level), dtype=torch.int32, device=self.device)
        self.cols = self.tile_cols * self.n_patches
        self.level = torch.as_tensor(level).to(self.device, torch.int32).contiguous().clone()
        self.type = torch.as_tensor(types).to(self.device, torch.int32).contiguous().clone()
        self.tile_origins = torch.as_tensor(tile_origins).to(self.device, torch.float32).reshape(-1, 2).contiguous().clone()
        self.origins = self.tile_origins if fp is None else fp.xy.view(-1, 2)
        if self.rows < 1 or self.cols < 1 or self.origins.shape[0] != self.rows * self.cols or self.level.shape != self.type.shape or self.level.dim() != 1:
            raise ValueError(f"terrain levels: {self.rows} x {self.cols} tiles need origins [{self.rows * self.cols}, 2] and level / type of one length")
        if self.level.numel() and (int(self.level.min()) < 0 or int(self.level.max()) >= self.rows or int(self.type.min()) < 0
                                   or int(self.type.max()) >= self.cols):
            raise ValueError(f"terrain levels outside [0, {self.rows}) or types outside [0, {self.cols})")
        self.struct = A.WlTerrainLevels(self.level.data_ptr(), self.type.data_ptr(), self.origins.data_ptr(), self.rows, self.cols)
        self.redeal(0)

    def redeal(self, epoch: int):
        """deal every env a slot of its column again (wl_flat_patch_deal on the current stream: no host work, no synchronisation);
        the slot counts from the env's next reset on.  Without flat patches: nothing to deal."""
        if self.patches is None:
            return
        A.check(A.load().wl_flat_patch_deal(self.type.shape[0], self.env_offset, self.world_envs, self.tile_cols, self.n_patches, int(epoch),
                                            self.seed, self.type.data_ptr(), A.stream(self.device)), "wl_flat_patch_deal")

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

    def env_origins_xy(self) -> torch.Tensor:
        """[n, 2]: the centre of every env's tile as the levels stand"""
        return self.origins[self.level.long() * self.cols + self.type.long()]

    def mean_level(self) -> torch.Tensor:
        """0-dim device tensor: what the terrain_levels curriculum term reports"""
        return self.level.float().mean()


def assemble_terrain(extra, cmd_xy: float, n_envs: int, device, env_offset: int = 0, world_envs: int | None = None, seed: int = 42):
    """The terrain of envs env_offset .. env_offset + n_envs of a world of `world_envs`, from the terrain entries of a flattened config
    (envs.flatten: `extra`, only read) -> (heightfield, levels, flat_patches) as ElevBatch takes them.  `heightfield`: the mesh
    rasterised, the generator's field, else the entry itself -- a DeviceHeightField whenever patches are found, for they live on it.
    `flat_patches`: {name: FlatPatches}.  `levels`: the curriculum's tables or None; where resets spawn on "init_pos" patches the
    tables carry them as virtual columns, with or without a curriculum (`cmd_xy`: the goal square that must then fit the lattice)."""
    import zlib
    gen, spec, curriculum = extra.get("terrain_generator"), extra.get("flat_patches"), extra.get("terrain_levels")
    hf = extra.get("heightfield")
    if extra.get("mesh_path") is not None:      # a mesh terrain: rasterised once, then a heightfield like any other
        hf = mesh_heightfield(*load_obj(extra["mesh_path"]), extra["mesh_cell"], device=device)
    if gen is not None:                         # a procedural terrain: generated on the device, redrawn in place
        hf = generate_heightfield(gen, device)
    found = {}
    if spec is not None:
        if not isinstance(hf, DeviceHeightField):      # the field the batch will share
            hf = DeviceHeightField(hf if hf is not None else synthetic_heightfield(), device)
        for name in spec["names"]:
            # one key per name: sets with equal sampling must not coincide ("init_pos" keeps the env's seed)
            key = seed if name == "init_pos" else (seed & 0xFFFFFFFF) | (zlib.crc32(name.encode()) << 32)
            found[name] = find_flat_patches(hf, gen if gen is not None else spec["sampling"][name], key, name)
    fp = found["init_pos"] if spec is not None and spec["spawn"] else None
    where = dict(device=device, env_offset=env_offset, world_envs=world_envs, seed=seed)
    if curriculum is not None:                  # each shard builds its slice of the world's assignment
        levels = TerrainLevels(gen, n_envs, max_init_terrain_level=curriculum["max_init_terrain_level"], flat_patches=fp, **where)
    elif fp is None:
        levels = None
    elif gen is not None:
        from .envs.terrain_levels import tile_origins
        levels = TerrainLevels.on_patches(fp, n_envs, 1, fp.n_tiles, tile_origins=tile_origins(gen), grid=(int(gen.num_rows), int(gen.num_cols)), **where)
    else:
        from .envs.flatten import check_patch_goals
        check_patch_goals(fp.table, hf.struct.nx, hf.struct.ny, hf.cell, cmd_xy)
        levels = TerrainLevels.on_patches(fp, n_envs, **where)
    return hf, levels, found
