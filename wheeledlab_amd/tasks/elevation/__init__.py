from .mushr_elevation_env_cfg import MushrElevationPlayEnvCfg, MushrElevationRLEnvCfg, MushrElevationTerrainLevelsEnvCfg  # noqa: F401
