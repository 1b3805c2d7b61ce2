"""Raw sensors to depth, point cloud and pictures in ONE captured graph: the camera front end, the radar front end, the input
assembly, the eval-mode network, the point-cloud back end (with the bird's-eye-view grid, the occupancy map, its objects, its distance
field and the navigation field behind it, if asked for) and the visualiser on static buffers, replayed once per frame.

Each stage exists on its own (camera.camera_inputs, radar.radar_inputs, batch.assemble_batch, inference.InferenceGraph,
cloud.point_cloud, viz.Visualizer) and LivePipeline.run returns the bits of calling them one by one; what it adds is the ownership of
every buffer between sensor and picture and one replay in place of a host call per stage: INTEGRATION.md, "Live pipeline".  The lidar
ground-truth front end serves training and is not part of it.  Nothing calls this module unless asked."""
import math

import torch

from . import field as fld
from . import lib as L
from . import match as mt
from . import nav as nv
from . import objects as obj
from . import occupancy as occ
from . import rollout as ro
from . import terrain as ter
from . import tracks as trk
from .bev import GRID_OPTIONS, BevWorkspace, bev_grid, grid_shape, picture
from .camera import ORDERS, camera_inputs
from .cloud import CloudWorkspace, point_cloud
from .radar import RadarWorkspace, radar_inputs
from ._frontend import _size, map_shape
from .viz import Visualizer

CLOUD_OPTIONS = {"stride": 1, "min_range": 0.0, "max_range": math.inf, "max_depth": 100.0, "rgb": False, "pixel": False}
BEV_OPTIONS = dict(GRID_OPTIONS, picture=False, picture_z_range=(-2.0, 4.0), cmap="jet")
# the map's own options (OccupancyMap), M (None: one map per frame; 1: the frames are the cameras of one rig), centre (None: the
# camera; or a point of the out frame the window is centred on, such as (20, 0, 0)) and picture (True: also occupancy.picture in cmap)
OCCUPANCY_OPTIONS = dict(occ.MAP_OPTIONS, nx=160, ny=160, cell=0.5, M=None, centre=None, picture=False, cmap="jet")
# the FieldSpec's own options (its cell is the map's), picture (True: also field.picture in cmap), paths ((K, P): also check_paths on K
# trajectories of P poses that run(paths=) brings) with blocked_at and outside_blocks
FIELD_OPTIONS = dict(fld.SPEC_OPTIONS, picture=False, cmap="jet", paths=None, blocked_at=253, outside_blocks=True)
# the NavSpec's own options (its cell is the map's), goals (G: the goal points of each map that run(goals=) brings) and starts ((K, P):
# also plan_paths from K starts that run(starts=) brings, at most P cells each) with xy (the paths' cell centres as well)
NAV_OPTIONS = dict(nv.SPEC_OPTIONS, goals=1, starts=None, xy=True)
# the ObjectSpec's own options (its cell is the map's)
OBJECT_OPTIONS = obj.SPEC_OPTIONS
# the TrackSpec's own options (the tracks take the map's shape and cell and the object table's rows)
TRACK_OPTIONS = trk.SPEC_OPTIONS
# the MatchSpec's own options (the matcher takes the map, its cell and its min_points unless given)
MATCH_OPTIONS = mt.SPEC_OPTIONS
# the RolloutSpec's own options but cell, which is the map's, tables (the per-candidate tables as well) and xy (the rollouts in the map frame)
ROLLOUT_OPTIONS = dict({k: v for k, v in ro.SPEC_OPTIONS.items() if k != "cell"}, tables=False, xy=False)
# the TerrainMap's own options (M, nx, ny and cell are the occupancy map's), picture (True: also terrain.picture over picture_z_range in
# cmap) and feeds_field (True: the distance field and what follows it read the terrain's state in place of the occupancy map's)
TERRAIN_OPTIONS = dict(ter.MAP_OPTIONS, picture=False, picture_z_range=(-2.0, 4.0), cmap="jet", feeds_field=False)
RADAR_ARGS = ("points", "sweep_index", "frame_offsets", "cam1_from_sensor", "cam2_from_sensor", "lags")


def _copies(v):
    if torch.is_tensor(v):
        return v.clone()
    if isinstance(v, dict):
        return {k: _copies(t) for k, t in v.items()}
    if isinstance(v, tuple):
        return tuple(_copies(t) for t in v)
    return v


class LivePipeline:
    """model.eval() on raw sensor data for a fixed batch of B frames of image_size pixels, captured once on one stream.

    model: a CamRaDepth on the device with input_channels 7 (image, radar depth, radar flow, radial velocity), 6 (without the radial
    velocity) or 3 (RGB only: run() then takes no radar arguments and the camera kernel writes the network input directly).
    (h, w) = map_shape(image_size, downsample_scale, y_cutoff) must be a shape the network takes (multiples of 32).  max_points and
    max_sweeps: the capacity of the radar tables (every run may bring fewer).  frame_channels, order_in: the raw frames' bytes per
    pixel (3 or 4) and channel order; order_out: the order the network was trained on ('bgr', as cv2 reads).  max_depth, min_distance,
    min_z: as for assemble_batch and radar_inputs.
    cloud: None, or a dictionary of point_cloud's stride, min_range, max_range, max_depth, rgb (colours from the image) and pixel.
    bev: None, or a dictionary of bev_grid's x_range, y_range, cell, z_range, min_points and flip, and picture (True: also the height
    map in colours, bev.picture over picture_z_range in cmap).  It needs cloud=: the grid is laid in the cloud's frame, out_from_cam.
    occupancy: None, or a dictionary of OCCUPANCY_OPTIONS: an OccupancyMap (`occupancy_map`, owned by this object) fused over the runs,
    fed from the cloud with the pose run(map_from_out=) brings.  It needs cloud=; the camera's position in the cloud's frame is the
    sensor.  The map is empty after construction; occupancy_map.reset() empties it again.
    field: None, or a dictionary of FIELD_OPTIONS: the distance field of the occupancy map's `state` (field.distance_field), with
    picture and paths=(K, P) also field.picture and field.check_paths.  It needs occupancy=, whose cell it takes.  The trajectories
    live in `paths_xy`, fp64 [K,P,2] (all NaN after construction: every pose outside), which run(paths=) fills; `path_n_poses` and
    `path_map`, int32 [K] (all P poses, map 0), are the caller's to change in place.
    nav: None, or a dictionary of NAV_OPTIONS: the navigation field of the distance field's costmap (nav.nav_field) towards goals=G
    goal points per map, with starts=(K, P) also nav.plan_paths.  It needs field=, whose costmap and cell it takes.  The goals live in
    `nav_goals`, fp64 [M,G,2], and the starts in `nav_starts`, fp64 [K,2] (all NaN after construction: no goal, and every path has
    status 2), which run(goals=, starts=) fill; `nav_n_goals`, int32 [M] (all G), and `nav_path_map`, int32 [K] (map 0), are the
    caller's to change in place.
    objects: None, or a dictionary of OBJECT_OPTIONS: the connected obstacles of the occupancy map's `state` as a label map and a
    table (objects.map_objects).  It needs occupancy=, whose cell it takes, and not field=.
    tracks: None, or a dictionary of TRACK_OPTIONS: the objects followed over the runs with ids that stay (tracks.track_objects on an
    ObjectTracks, `object_tracks`, owned by this object).  It needs objects=, with max_objects <= 1024.  The tracks are empty after
    construction; object_tracks.reset() empties them again.
    match: None, or a dictionary of MATCH_OPTIONS: the pose run(map_from_out=) brings is corrected against the occupancy map as it stands
    (match.match_scan) before the cloud is fused, and the update reads the corrected pose.  It needs occupancy=.  The first run finds
    the map empty and passes the pose through, with match.UNINITIALISED in its status.
    viz: None, or a dictionary of Visualizer's options (image_order is order_out unless given).
    rollout: None, or a dictionary of ROLLOUT_OPTIONS: the local planner (rollout.plan_rollouts) on the distance field's costmap, with
    the cost-to-go of nav= and the tracks of tracks= when they are there, from the pose the occupancy update read (the matcher's with
    match=; frame 0's when the frames share one map).  It needs field=, whose cell it takes.  With accel= the current (v, w) lives in
    `rollout_twist`, fp64 [M,2] (zeros after construction), which run(twist=) fills.
    terrain: None, or a dictionary of TERRAIN_OPTIONS: a TerrainMap (`terrain_map`, owned by this object) of the occupancy map's M, nx,
    ny and cell, fused over the runs from the same cloud, pose (the matcher's with match=), sensor and centre as the occupancy map, so
    their origins are equal.  It needs occupancy=.  With feeds_field=True the distance field, and with it check_paths, nav_field,
    plan_paths and plan_rollouts, read the terrain's state where they read the occupancy map's; objects= and tracks= keep reading the
    occupancy map.  The map is empty after construction; terrain_map.reset() empties it again.

    The graph holds, in this order and without a parallel branch: crd_camera_frontend, radar_inputs, crd_assemble_input into the
    plan's input buffer, the network's forward (weights are packed before a replay when they changed, not inside the graph),
    point_cloud, bev_grid [, bev.picture] [, match.match_scan], occupancy.update [, occupancy.picture] [, terrain.update [, terrain.picture]] [, objects.map_objects [, tracks.track_objects]], field.distance_field [, field.picture] [,
    field.check_paths] [, nav.nav_field [, nav.plan_paths]], Visualizer.render [, rollout.plan_rollouts]."""

    def __init__(self, model, B, image_size=(900, 1600), downsample_scale=2, y_cutoff=34, max_points=None, max_sweeps=None,
                 frame_channels=3, order_in="rgb", order_out="bgr", max_depth=100.0, min_distance=1.0, min_z=2.0, cloud=None, viz=None,
                 bev=None, occupancy=None, field=None, nav=None, objects=None, tracks=None, match=None, rollout=None, terrain=None):
        fn = "LivePipeline"
        if terrain is not None:
            if occupancy is None:
                raise L.CrdError(f"{fn}: terrain= needs occupancy= (the terrain map takes the occupancy map's window, pose and cell)")
            if not isinstance(terrain, dict) or not set(terrain) <= set(TERRAIN_OPTIONS):
                raise L.CrdError(f"{fn}: terrain= holds {sorted(TERRAIN_OPTIONS)}, not {terrain!r}")
        if rollout is not None:
            if field is None:
                raise L.CrdError(f"{fn}: rollout= needs field= (the rollouts are tested on the distance field's costmap)")
            if not isinstance(rollout, dict) or not set(rollout) <= set(ROLLOUT_OPTIONS):
                raise L.CrdError(f"{fn}: rollout= holds {sorted(ROLLOUT_OPTIONS)}, not {rollout!r}")
        if match is not None:
            if occupancy is None:
                raise L.CrdError(f"{fn}: match= needs occupancy= (the pose is matched against the map)")
            if not isinstance(match, dict) or not set(match) <= set(MATCH_OPTIONS):
                raise L.CrdError(f"{fn}: match= holds {sorted(MATCH_OPTIONS)}, not {match!r}")
        if tracks is not None:
            if objects is None:
                raise L.CrdError(f"{fn}: tracks= needs objects= (the tracks follow the rows of the object table)")
            if not isinstance(tracks, dict) or not set(tracks) <= set(TRACK_OPTIONS):
                raise L.CrdError(f"{fn}: tracks= holds {sorted(TRACK_OPTIONS)}, not {tracks!r}")
        if objects is not None:
            if occupancy is None:
                raise L.CrdError(f"{fn}: objects= needs occupancy= (the objects are those of the map's state, with its cell)")
            if not isinstance(objects, dict) or not set(objects) <= set(OBJECT_OPTIONS):
                raise L.CrdError(f"{fn}: objects= holds {sorted(OBJECT_OPTIONS)}, not {objects!r}")
        if nav is not None:
            if field is None:
                raise L.CrdError(f"{fn}: nav= needs field= (the navigation field is made from the distance field's costmap)")
            if not isinstance(nav, dict) or not set(nav) <= set(NAV_OPTIONS):
                raise L.CrdError(f"{fn}: nav= holds {sorted(NAV_OPTIONS)}, not {nav!r}")
        if field is not None:
            if occupancy is None:
                raise L.CrdError(f"{fn}: field= needs occupancy= (the field is made from the map's state, with its cell)")
            if not isinstance(field, dict) or not set(field) <= set(FIELD_OPTIONS):
                raise L.CrdError(f"{fn}: field= holds {sorted(FIELD_OPTIONS)}, not {field!r}")
        if occupancy is not None:
            if cloud is None:
                raise L.CrdError(f"{fn}: occupancy= needs cloud= (the map is fed from the point cloud)")
            if not isinstance(occupancy, dict) or not set(occupancy) <= set(OCCUPANCY_OPTIONS):
                raise L.CrdError(f"{fn}: occupancy= holds {sorted(OCCUPANCY_OPTIONS)}, not {occupancy!r}")
        if bev is not None:
            if cloud is None:
                raise L.CrdError(f"{fn}: bev= needs cloud= (the grid is made from the point cloud, in its frame)")
            if not isinstance(bev, dict) or not set(bev) <= set(BEV_OPTIONS):
                raise L.CrdError(f"{fn}: bev= holds {sorted(BEV_OPTIONS)}, not {bev!r}")
        if model.flat is None or not model.flat.is_cuda:
            raise L.CrdError(f"{fn} needs the model on an MI355X (no CPU fallback)")
        Cin = model.cfg.input_channels
        if Cin not in (3, 6, 7):
            raise L.CrdError(f"{fn}: a model of {Cin} input channels; 7, 6 (image and radar) or 3 (image only) are assembled here")
        if order_in not in ORDERS or order_out not in ORDERS:
            raise L.CrdError(f"{fn}: order_in and order_out are 'rgb' or 'bgr', not {order_in!r} and {order_out!r}")
        if frame_channels not in (3, 4) or int(B) <= 0:
            raise L.CrdError(f"{fn}: B {B}, frame_channels {frame_channels} (3 or 4)")
        h, w = map_shape(image_size, downsample_scale, y_cutoff)
        if h % 32 or w % 32:
            raise L.CrdError(f"{fn}: image {tuple(image_size)}, downsample_scale {downsample_scale}, y_cutoff {y_cutoff} give maps of "
                             f"{h} x {w}; the network takes multiples of 32")
        self.radar_on = Cin > 3
        if self.radar_on and (max_points is None or max_sweeps is None or int(max_points) <= 0 or int(max_sweeps) <= 0):
            raise L.CrdError(f"{fn}: a model with radar channels needs max_points and max_sweeps, the capacity of the radar tables")
        if cloud is not None and not set(cloud) <= set(CLOUD_OPTIONS):
            raise L.CrdError(f"{fn}: cloud= holds {sorted(CLOUD_OPTIONS)}, not {sorted(set(cloud) - set(CLOUD_OPTIONS))}")
        dev = model.flat.device
        self.model, self.B, self.h, self.w = model, int(B), h, w
        self.image_size, self.downsample_scale, self.y_cutoff = _size(image_size), int(downsample_scale), int(y_cutoff)
        self.order_in, self.order_out, self.max_depth = order_in, order_out, float(max_depth)
        self.min_distance, self.min_z = float(min_distance), float(min_z)
        H, W = self.image_size
        B = self.B
        # every static buffer between sensor and picture
        self.frames = torch.zeros(B, H, W, int(frame_channels), dtype=torch.uint8, device=dev)
        self.image = torch.empty(B, h, w, 3, dtype=torch.uint8, device=dev)
        self.K = torch.eye(3, dtype=torch.float64, device=dev).repeat(B, 1, 1)
        self.camera_frame = torch.eye(3, 4, dtype=torch.float64, device=dev).repeat(B, 1, 1)       # out_from_cam=None: (I | 0)
        self.out_from_cam = self.camera_frame.clone()
        if self.radar_on:
            N, S = int(max_points), int(max_sweeps)
            self.max_points, self.max_sweeps = N, S
            self.points = torch.zeros(N, 5, dtype=torch.float64, device=dev)
            self.sweep_index = torch.zeros(N, dtype=torch.int32, device=dev)
            self.frame_offsets = torch.zeros(B + 1, dtype=torch.int32, device=dev)
            self.cam1_from_sensor = torch.zeros(S, 3, 4, dtype=torch.float64, device=dev)
            self.cam2_from_sensor = torch.zeros(S, 3, 4, dtype=torch.float64, device=dev)
            self.lags = torch.zeros(S, 2, dtype=torch.float64, device=dev)
            self.radar_ws = RadarWorkspace(B, self.image_size, self.downsample_scale, max_points=N, device=dev)
            self.radar_out = {"radar": torch.empty(B, h, w, 3, device=dev), "rad_vel": torch.empty(B, h, w, device=dev)}
        self.cloud_opts = None if cloud is None else dict(CLOUD_OPTIONS, **cloud)
        if self.cloud_opts is not None:
            self.cloud_ws = CloudWorkspace(B, self.image_size, self.downsample_scale, self.y_cutoff, self.cloud_opts["stride"], device=dev)
            self.cloud_out = self.cloud_ws.outputs(rgb=bool(self.cloud_opts["rgb"]), pixel=bool(self.cloud_opts["pixel"]))
        self.bev_opts = None if bev is None else dict(BEV_OPTIONS, **bev)
        if self.bev_opts is not None:
            o = self.bev_opts
            nx, ny = grid_shape(o["x_range"], o["y_range"], o["cell"])
            self.bev_ws = BevWorkspace(B, nx, ny, device=dev)
            self.bev_out = self.bev_ws.outputs()
            self.bev_picture = torch.empty(B, nx, ny, 3, dtype=torch.uint8, device=dev) if o["picture"] else None
        self.occupancy_opts = None if occupancy is None else dict(OCCUPANCY_OPTIONS, **occupancy)
        self.occupancy_map = None
        if self.occupancy_opts is not None:
            o = self.occupancy_opts
            self.occupancy_map = occ.OccupancyMap(B if o["M"] is None else o["M"], o["nx"], o["ny"], o["cell"], device=dev,
                                                  **{k: o[k] for k in occ.MAP_OPTIONS})
            self.occupancy_ws = occ.OccupancyWorkspace(self.occupancy_map, B)
            self.map_from_out = self.camera_frame.clone()
            self.sensor = torch.zeros(B, 3, dtype=torch.float64, device=dev)
            try:
                centre = None if o["centre"] is None else [float(v) for v in o["centre"]]
            except (TypeError, ValueError):
                centre = ()
            if centre is not None and len(centre) != 3:
                raise L.CrdError(f"{fn}: occupancy centre {o['centre']!r} is three numbers")
            self.centre = None if centre is None else torch.tensor(centre, dtype=torch.float64, device=dev)
            M = self.occupancy_map.M
            self.occupancy_picture = torch.empty(M, o["nx"], o["ny"], 3, dtype=torch.uint8, device=dev) if o["picture"] else None
        self.terrain_opts = None if terrain is None else dict(TERRAIN_OPTIONS, **terrain)
        self.terrain_map = None
        if self.terrain_opts is not None:
            o, omap = self.terrain_opts, self.occupancy_map
            self.terrain_map = ter.TerrainMap(omap.M, omap.nx, omap.ny, omap.cell, device=dev, **{k: o[k] for k in ter.MAP_OPTIONS})
            self.terrain_ws = ter.TerrainWorkspace(self.terrain_map, B)
            self.terrain_picture = torch.empty(omap.M, omap.nx, omap.ny, 3, dtype=torch.uint8, device=dev) if o["picture"] else None
        self.match_spec = None
        if match is not None:
            self.match_spec = mt.MatchSpec(device=dev, **dict(MATCH_OPTIONS, **match))
            self.match_ws = mt.MatchWorkspace(self.occupancy_map, self.match_spec, B)
        self.object_spec = None
        if objects is not None:
            omap = self.occupancy_map
            self.object_spec = obj.ObjectSpec(omap.cell, **dict(OBJECT_OPTIONS, **objects))
            self.object_ws = obj.ObjectWorkspace(self.object_spec, omap.M, omap.nx, omap.ny, device=dev)
        self.track_spec, self.object_tracks = None, None
        if tracks is not None:
            omap = self.occupancy_map
            self.track_spec = trk.TrackSpec(**dict(TRACK_OPTIONS, **tracks))
            self.object_tracks = trk.ObjectTracks(self.track_spec, omap.M, omap.nx, omap.ny, omap.cell, device=dev)
            self.track_ws = trk.TrackWorkspace(self.track_spec, self.object_tracks, self.object_spec.max_objects)
        self.field_opts = None if field is None else dict(FIELD_OPTIONS, **field)
        self.field_spec = None
        if self.field_opts is not None:
            o, omap = self.field_opts, self.occupancy_map
            self.field_spec = fld.FieldSpec(omap.cell, device=dev, **{k: o[k] for k in fld.SPEC_OPTIONS})
            self.field_ws = fld.FieldWorkspace(self.field_spec, omap.M, omap.nx, omap.ny)
            self.field_picture = torch.empty(omap.M, omap.nx, omap.ny, 3, dtype=torch.uint8, device=dev) if o["picture"] else None
            self.paths_xy = None
            if o["paths"] is not None:
                try:
                    K, P = (int(v) for v in o["paths"])
                except (TypeError, ValueError):
                    K = P = 0
                if K < 1 or P < 1:
                    raise L.CrdError(f"{fn}: field paths {o['paths']!r} is (K, P), paths and poses per path, each at least 1")
                self.paths_xy = torch.full((K, P, 2), math.nan, dtype=torch.float64, device=dev)
                self.path_n_poses = torch.full((K,), P, dtype=torch.int32, device=dev)
                self.path_map = torch.zeros(K, dtype=torch.int32, device=dev)
                self.paths_out = fld.path_outputs(K, P, device=dev)
        self.nav_opts = None if nav is None else dict(NAV_OPTIONS, **nav)
        self.nav_spec = None
        if self.nav_opts is not None:
            o, omap = self.nav_opts, self.occupancy_map
            self.nav_spec = nv.NavSpec(omap.cell, **{k: o[k] for k in nv.SPEC_OPTIONS})
            try:
                G = int(o["goals"])
                K, P = (0, 0) if o["starts"] is None else (int(v) for v in o["starts"])
            except (TypeError, ValueError):
                G = K = P = -1
            if G < 1 or (o["starts"] is not None and (K < 1 or P < 1)):
                raise L.CrdError(f"{fn}: nav goals {o['goals']!r} is G >= 1, goals per map, and starts {o['starts']!r} is None or (K, P), paths "
                                 "and cells per path, each at least 1")
            self.nav_ws = nv.NavWorkspace(self.nav_spec, omap.M, omap.nx, omap.ny, device=dev)
            self.nav_goals = torch.full((omap.M, G, 2), math.nan, dtype=torch.float64, device=dev)
            self.nav_n_goals = torch.full((omap.M,), G, dtype=torch.int32, device=dev)
            self.nav_starts = None
            if o["starts"] is not None:
                self.nav_P = P
                self.nav_starts = torch.full((K, 2), math.nan, dtype=torch.float64, device=dev)
                self.nav_path_map = torch.zeros(K, dtype=torch.int32, device=dev)
                self.nav_paths_out = nv.path_outputs(K, P, xy=bool(o["xy"]), device=dev)
        self.rollout_spec = None
        if rollout is not None:
            o, omap = dict(ROLLOUT_OPTIONS, **rollout), self.occupancy_map
            self.rollout_opts = o
            self.rollout_spec = ro.RolloutSpec(device=dev, cell=omap.cell, **{k: o[k] for k in ro.SPEC_OPTIONS if k != "cell"})
            self.rollout_ws = ro.RolloutWorkspace(self.rollout_spec, omap.M, tables=bool(o["tables"]), xy=bool(o["xy"]))
            self.rollout_twist = None
            if self.rollout_spec.accel is not None:
                self.rollout_twist = torch.zeros(omap.M, 2, dtype=torch.float64, device=dev)
        self.visualizer = None if viz is None else Visualizer(B, h, w, **dict({"image_order": order_out, "device": dev}, **viz))
        # the eval plan, exactly as InferenceGraph takes it
        was_training = model.training
        model.eval()
        prev = model.__dict__.get("_need_grad", True)
        model.__dict__["_need_grad"] = False        # inference: nothing is kept for a backward pass
        try:
            self.plan = model._plan_for(torch.zeros((B, Cin, h, w), device=dev))
        finally:
            model.__dict__["_need_grad"] = prev     # (part of the plan key: a later model._plan_for() must not inherit it)
        self.stream = torch.cuda.Stream()
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            self._stages(pack=True)                 # warm-up outside the capture (lazy module loading)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.stream):
                self._results = self._stages(pack=False)
            if self.occupancy_map is not None:      # the warm-up pass fused a frame of zeros into the map: the first run starts empty
                self.occupancy_map.reset()
                self.occupancy_map.status_word.zero_()
            if self.terrain_map is not None:        # and into the terrain map
                self.terrain_map.reset()
                self.terrain_map.status_word.zero_()
            if self.object_tracks is not None:      # and gave its objects tracks
                self.object_tracks.reset()
        torch.cuda.current_stream().wait_stream(self.stream)
        model.train(was_training)

    def _pred(self):
        """The reference's nested output dictionary as views of the plan's static buffers (InferenceGraph.run(clone=False))."""
        p, B, H, W = self.plan, self.B, self.h, self.w
        final = p.out_depth[5].t.view(B, 1, H, W)
        half = p.out_depth[4].t.view(B, 1, H // 2, W // 2)
        quarter = p.out_depth[3].t.view(B, 1, H // 4, W // 4)
        return {"depth": {"intermediate_depths": (None, None, quarter, half), "final_depth": final},
                "seg": {"final_seg": p.seg_out if p.seg_logits is not None else None, "intermediate_seg": None, "unsup_map": p.unsup_map}}

    def _stages(self, pack):
        """The whole chain on the current stream, every stage writing into this object's buffers -> the dictionary run() returns."""
        p, s, cut = self.plan, self.downsample_scale, self.y_cutoff
        out = {"x": p.x_in}
        if self.radar_on:
            out["image"] = camera_inputs(self.frames, s, cut, self.order_in, self.order_out, out={"image": self.image})["image"]
            maps = radar_inputs(self.points, self.sweep_index, self.frame_offsets, self.cam1_from_sensor, self.cam2_from_sensor, self.lags,
                                self.K, self.image_size, self.min_distance, self.min_z, s, cut, workspace=self.radar_ws, out=self.radar_out)
            rad_vel = maps["rad_vel"] if p.x_in.shape[1] == 7 else None
            L.check(p.lib.crd_assemble_input(L.ptr(self.image), L.ptr(maps["radar"]), L.ptr(rad_vel), self.B, self.h, self.w, self.max_depth,
                                             L.ptr(p.x_in), L.stream()), "crd_assemble_input")
            out.update(radar=maps["radar"], rad_vel=maps["rad_vel"])
        else:
            out["image"] = camera_inputs(self.frames, s, cut, self.order_in, self.order_out, out={"image": self.image, "x": p.x_in})["image"]
        p.forward(pack=pack)
        pred = out["pred"] = self._pred()
        if self.cloud_opts is not None:
            o = self.cloud_opts
            out["cloud"] = point_cloud(pred["depth"]["final_depth"], self.K, self.image_size, s, cut, o["max_depth"],
                                       out_from_cam=self.out_from_cam, min_range=o["min_range"], max_range=o["max_range"], stride=o["stride"],
                                       image=self.image if o["rgb"] else None, with_pixel=bool(o["pixel"]), workspace=self.cloud_ws,
                                       out=self.cloud_out)
            if self.bev_opts is not None:
                o = self.bev_opts
                grid = bev_grid(out["cloud"], x_range=o["x_range"], y_range=o["y_range"], cell=o["cell"], z_range=o["z_range"],
                                min_points=o["min_points"], flip=o["flip"], workspace=self.bev_ws, out=self.bev_out)
                out["bev"] = dict(grid)
                if self.bev_picture is not None:
                    out["bev"]["picture"] = picture(grid, o["picture_z_range"], o["cmap"], out=self.bev_picture)
            if self.occupancy_map is not None:
                pose = self.map_from_out
                if self.match_spec is not None:
                    out["match"] = dict(mt.match_scan(self.occupancy_map, self.match_spec, out["cloud"], map_from_points=pose, sensor=self.sensor,
                                                      workspace=self.match_ws))
                    pose = out["match"]["pose"]
                res = occ.update(self.occupancy_map, out["cloud"], map_from_points=pose, sensor=self.sensor, centre=self.centre,
                                 workspace=self.occupancy_ws, out=self.occupancy_ws.out)
                out["occupancy"] = dict(res)
                if self.occupancy_picture is not None:
                    out["occupancy"]["picture"] = occ.picture(res, self.occupancy_map, self.occupancy_opts["cmap"], out=self.occupancy_picture)
                grid = res                          # whose state and origin the field and what follows it read
                if self.terrain_map is not None:
                    o = self.terrain_opts
                    land = ter.update(self.terrain_map, out["cloud"], map_from_points=pose, sensor=self.sensor, centre=self.centre,
                                      workspace=self.terrain_ws, out=self.terrain_ws.out)
                    out["terrain"] = dict(land)
                    if self.terrain_picture is not None:
                        out["terrain"]["picture"] = ter.picture(land, o["picture_z_range"], o["cmap"], out=self.terrain_picture)
                    if o["feeds_field"]:
                        grid = land
                if self.object_spec is not None:
                    out["objects"] = dict(obj.map_objects(self.object_spec, res, res, workspace=self.object_ws))
                    if self.track_spec is not None:
                        out["tracks"] = dict(trk.track_objects(self.track_spec, self.object_tracks, out["objects"], res,
                                                               workspace=self.track_ws))
                if self.field_spec is not None:
                    o = self.field_opts
                    dist = fld.distance_field(self.field_spec, grid, workspace=self.field_ws, out=self.field_ws.out)
                    out["field"] = dict(dist)
                    if self.field_picture is not None:
                        out["field"]["picture"] = fld.picture(dist, self.field_spec, o["cmap"], out=self.field_picture)
                    if self.paths_xy is not None:
                        out["field"]["paths"] = dict(fld.check_paths(self.field_spec, dist, grid, self.paths_xy, self.path_n_poses, self.path_map,
                                                                     blocked_at=o["blocked_at"], outside_blocks=o["outside_blocks"],
                                                                     out=self.paths_out))
                    if self.nav_spec is not None:
                        field_to_go = nv.nav_field(self.nav_spec, dist, grid, self.nav_goals, self.nav_n_goals, workspace=self.nav_ws)
                        out["nav"] = dict(field_to_go)
                        if self.nav_starts is not None:
                            out["nav"]["paths"] = dict(nv.plan_paths(self.nav_spec, field_to_go, grid, self.nav_starts, self.nav_P,
                                                                     self.nav_path_map, xy=bool(self.nav_opts["xy"]), out=self.nav_paths_out))
        if self.visualizer is not None:
            out["pictures"] = self.visualizer.render(self.image, p.x_in if self.radar_on else None, pred)
        if self.rollout_spec is not None:
            o, M = self.rollout_opts, self.occupancy_map.M
            out["rollout"] = dict(ro.plan_rollouts(self.rollout_spec, pose[:M], out["field"], grid, nav_result=out.get("nav"),
                                                   tracks=self.object_tracks, twist=self.rollout_twist, workspace=self.rollout_ws,
                                                   tables=bool(o["tables"]), xy=bool(o["xy"])))
        return out

    def _load(self, buf, value, what, rows=False):
        """value into the static buffer buf; rows: value may hold fewer leading rows than buf, the rest is left as it is."""
        if not torch.is_tensor(value):
            raise L.CrdError(f"LivePipeline.run: {what} must be a tensor")
        dst = buf
        if rows:
            if value.dim() != buf.dim() or value.shape[0] > buf.shape[0]:
                raise L.CrdError(f"LivePipeline.run: {what} {list(value.shape)} does not fit the capacity {list(buf.shape)}")
            dst = buf[:value.shape[0]]
        if value.dtype != buf.dtype or tuple(value.shape) != tuple(dst.shape):
            raise L.CrdError(f"LivePipeline.run: {what} must be {buf.dtype} {list(dst.shape)}, not {value.dtype} {list(value.shape)}")
        dst.copy_(value)

    def run(self, frames, points=None, sweep_index=None, frame_offsets=None, cam1_from_sensor=None, cam2_from_sensor=None, lags=None, K=None,
            out_from_cam=None, clone=False, map_from_out=None, paths=None, goals=None, starts=None, twist=None):
        """One batch of sensor data through the graph.

        frames: uint8 [B,H,W,frame_channels] with any strides (a view of a capture buffer; a host tensor is copied up).  points
        [n,5], sweep_index [n], frame_offsets [B+1], cam1_from_sensor / cam2_from_sensor [S,3,4], lags [S,2]: radar_inputs' arguments
        with n <= max_points and S <= max_sweeps, frame_offsets ending at or below n; a 3-channel model takes none of them.  K: fp64
        [3,3] or [B,3,3], the camera's intrinsics at full resolution (the radar projection and the cloud read it; an RGB-only pipeline
        without a cloud needs none).  out_from_cam: fp64 [3,4] or [B,3,4], the cloud's frame; None: the camera's own.  map_from_out:
        fp64 [3,4] or [B,3,4], the pose of the cloud's frame in the occupancy map's frame for this batch (with occupancy= only); None:
        the identity.  paths: fp64 [K,P,2], the trajectories of this batch in the map frame (with field=dict(paths=(K, P)) only);
        None: those of the run before.  goals: fp64 [M,G,2], the goal points of this batch in the map frame (with nav= only), and
        starts: fp64 [K,2], the starts of its planned paths (with nav=dict(starts=(K, P)) only); None: those of the run before.  twist: fp64 [M,2], the vehicle's current (v, w)
        (with rollout=dict(accel=(a_v, a_w)) only); None: that of the run before.

        Returns 'image' (uint8 [B,h,w,3]), 'x' (the network input), 'radar' and 'rad_vel' (with radar), 'pred' (the reference's nested
        output dictionary), 'cloud', 'bev', 'match', 'occupancy', 'terrain', 'objects', 'tracks', 'field', 'nav', 'pictures' and 'rollout' (if asked for at construction: the
        dictionaries of point_cloud, of bev_grid, of match.match_scan, of occupancy.update, of terrain.update, of objects.map_objects, of tracks.track_objects and of field.distance_field -- each with 'picture' if asked for, the last with
        'paths', check_paths' dictionary --, of nav.nav_field -- with 'paths', plan_paths' dictionary --, of Visualizer.render and of rollout.plan_rollouts).  They are VIEWS of this
        object's static buffers, valid until the
        next run(), which overwrites them in place; clone=True returns copies.  Nothing is allocated (with clone=False) and the call
        does not wait for the device."""
        self._load(self.frames, frames, "frames")
        radar_args = (points, sweep_index, frame_offsets, cam1_from_sensor, cam2_from_sensor, lags)
        if self.radar_on:
            if not all(torch.is_tensor(v) for v in radar_args) or K is None:
                raise L.CrdError(f"LivePipeline.run: a model with radar channels takes the tensors {', '.join(RADAR_ARGS)} and K")
            if points.shape[0] != sweep_index.shape[0] or not (cam1_from_sensor.shape[0] == cam2_from_sensor.shape[0] == lags.shape[0]):
                raise L.CrdError(f"LivePipeline.run: {points.shape[0]} points with {sweep_index.shape[0]} sweep indices; sweep tables of "
                                 f"{cam1_from_sensor.shape[0]}, {cam2_from_sensor.shape[0]} and {lags.shape[0]} rows")
            for name, value in zip(RADAR_ARGS, radar_args):
                self._load(getattr(self, name), value, name, rows=name != "frame_offsets")
        elif any(v is not None for v in radar_args):
            raise L.CrdError("LivePipeline.run: an RGB-only model takes no radar arguments")
        if K is not None:
            self._load(self.K, K.expand(self.B, 3, 3) if torch.is_tensor(K) and tuple(K.shape) == (3, 3) else K, "K")
        elif self.cloud_opts is not None:
            raise L.CrdError("LivePipeline.run: the point cloud needs K")
        if out_from_cam is None:
            self.out_from_cam.copy_(self.camera_frame)
        else:
            self._load(self.out_from_cam, out_from_cam.expand(self.B, 3, 4) if torch.is_tensor(out_from_cam) and
                       tuple(out_from_cam.shape) == (3, 4) else out_from_cam, "out_from_cam")
        if self.occupancy_map is not None:
            self.sensor.copy_(self.out_from_cam[:, :, 3])                     # the camera's position in the cloud's frame
            if map_from_out is None:
                self.map_from_out.copy_(self.camera_frame)
            else:
                self._load(self.map_from_out, map_from_out.expand(self.B, 3, 4) if torch.is_tensor(map_from_out) and
                           tuple(map_from_out.shape) == (3, 4) else map_from_out, "map_from_out")
        elif map_from_out is not None:
            raise L.CrdError("LivePipeline.run: map_from_out goes with occupancy=")
        if paths is not None:
            if self.field_spec is None or self.paths_xy is None:
                raise L.CrdError("LivePipeline.run: paths goes with field=dict(paths=(K, P))")
            self._load(self.paths_xy, paths, "paths")
        if goals is not None:
            if self.nav_spec is None:
                raise L.CrdError("LivePipeline.run: goals goes with nav=")
            self._load(self.nav_goals, goals, "goals")
        if starts is not None:
            if self.nav_spec is None or self.nav_starts is None:
                raise L.CrdError("LivePipeline.run: starts goes with nav=dict(starts=(K, P))")
            self._load(self.nav_starts, starts, "starts")
        if twist is not None:
            if self.rollout_spec is None or self.rollout_twist is None:
                raise L.CrdError("LivePipeline.run: twist goes with rollout=dict(accel=(a_v, a_w))")
            self._load(self.rollout_twist, twist, "twist")
        self.plan.ensure_packed()                   # optimizer step / load_state_dict / mark_params_changed() since the last frame
        self.graph.replay()
        return _copies(self._results) if clone else dict(self._results)
