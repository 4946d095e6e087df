"""4D plans: the warps of the phases of a 4DCT as the records Engine.create_4d_optimizer, Engine.warp_sum_device and
Engine.warp_dose_t_phases_device take (include/rtd.h "4D dose: phases warped and summed")."""
from . import abi, grids


class PhaseWarps:
    """The records (abi.RtdWarp, one per phase) and the device fields they point to. The fields must outlive every optimiser made
    from the records: call free() after the optimiser is destroyed."""

    def __init__(self, engine, records, dev_fields):
        self.engine, self.records, self._dev = engine, records, dev_fields

    def __iter__(self):
        return iter(self.records)

    def __len__(self):
        return len(self.records)

    def __getitem__(self, i):
        return self.records[i]

    def free(self):
        self.engine.sync()
        for p in self._dev:
            self.engine.device_free(p)
        self._dev = []


def phase_warps(engine, ref_idx_to_world, phase_idx_to_world, dvfs, dvf_idx_to_world):
    """Uploads the fields and makes one rtd_warp per phase through grids.warp_maps. ref_idx_to_world, phase_idx_to_world: the
    index-to-world transforms of the reference grid and of the phases' dose grid (one grid for all phases); dvfs: one host field
    [3][Z][Y][X] float32 per phase, displacements in world mm at reference positions leading to the matching place of that phase;
    dvf_idx_to_world: the transform of the fields' grid (4x4 or an (M, v) pair) for all phases, or a dict {phase: transform} with
    one per phase (the fields may have different dims). -> PhaseWarps."""
    per_phase = isinstance(dvf_idx_to_world, dict)
    records, dev = [], []
    try:
        for p, dvf in enumerate(dvfs):
            to_world = dvf_idx_to_world[p] if per_phase else dvf_idx_to_world
            maps = grids.warp_maps(ref_idx_to_world, phase_idx_to_world, to_world)
            d, dims = engine._upload_dvf(dvf)
            dev.append(d)
            records.append(abi.make_warp(*maps, d, dims))
    except Exception:
        for d in dev:
            engine.device_free(d)
        raise
    return PhaseWarps(engine, records, dev)
