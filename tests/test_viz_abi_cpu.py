"""CPU: the C ABI of the visualisation back end without a GPU.  tests/test_abi.py parses the header against the library and the
binding and so covers the three new declarations; here every entry refuses bad arguments before any GPU call, with the documented
status and its own name in crd_last_error, and the Python interface refuses host tensors, wrong types and shapes and bad ranges."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crd_viz_range", "crd_viz_draw", "crd_seg_labels")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from camradepth_amd import lib
    return lib


def test_new_symbols_are_declared_exported_and_bound(built):
    h = open(os.path.join(REPO, "include", "camradepth_hip.h")).read()
    L = built.load()
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), f"{name} is not declared"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in built._SIGS and getattr(L, name).argtypes is not None, f"{name} is not bound"
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, h, flags=re.S).group(1)
        assert "double" not in args, name
    assert L.crd_version() == 13                                                               # no struct, no changed signature
    from camradepth_amd import viz
    assert viz.TILE == int(re.search(r"#define\s+CRD_VIZ_TILE\s+(\d+)", h).group(1))
    for name, value in (("CRD_VIZ_FLOAT", viz.FLOAT), ("CRD_VIZ_LABELS", viz.LABELS), ("CRD_VIZ_NONE", viz.MODES[None]),
                        ("CRD_VIZ_PASTE", viz.MODES["paste"]), ("CRD_VIZ_BLEND", viz.MODES["blend"]), ("CRD_VIZ_IMAGE", viz.MODES["image"])):
        assert value == int(re.search(r"#define\s+%s\s+(\d+)" % name, h).group(1)), name


def test_invalid_arguments_are_reported_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15

    def rng(**kw):
        v = dict(src=a, kind=0, B=2, h=416, w=800, dilate=0, dilated=None, ws=a, ws_bytes=1 << 40, range=a)
        v.update(kw)
        return L.crd_viz_range(v["src"], v["kind"], v["B"], v["h"], v["w"], v["dilate"], v["dilated"], v["ws"], v["ws_bytes"], v["range"], None)

    def draw(**kw):
        v = dict(src=a, kind=0, B=2, h=416, w=800, table=a, range=a, vmin=0.0, vmax=1.0, bad=0, image=None, bgr=1, mode=0, alpha=0.8, beta=0.75,
                 grey=0, out=a, row=2400, frame=2400 * 416)
        v.update(kw)
        return L.crd_viz_draw(v["src"], v["kind"], v["B"], v["h"], v["w"], v["table"], v["range"], v["vmin"], v["vmax"], v["bad"], v["image"],
                              v["bgr"], v["mode"], v["alpha"], v["beta"], v["grey"], v["out"], v["row"], v["frame"], None)

    def labels(**kw):
        v = dict(logits=a, B=2, C=21, h=416, w=800, labels=a)
        v.update(kw)
        return L.crd_seg_labels(v["logits"], v["B"], v["C"], v["h"], v["w"], v["labels"], None)

    def refused(rc, name, word, status=-1):
        msg = L.crd_last_error()
        assert rc == status and name in msg and word in msg, (rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, name.decode())

    inf, nan = float("inf"), float("nan")
    shapes = ((dict(B=0), b"bad argument"), (dict(B=-1), b"bad argument"), (dict(h=0), b"bad argument"), (dict(w=0), b"bad argument"),
              (dict(w=-5), b"bad argument"))
    for fn, name in ((rng, b"crd_viz_range"), (draw, b"crd_viz_draw"), (labels, b"crd_seg_labels")):
        for kw, word in shapes:
            refused(fn(**kw), name, word)
        refused(fn(h=1 << 16, w=1 << 15), name, b"unsupported", status=-2)            # 2^31 pixels per frame
    tiles = 2 * 325                                       # 416 x 800 pixels per frame in tiles of 1024
    for kw, word in ((dict(src=None), b"null"), (dict(ws=None), b"null"), (dict(range=None), b"null"), (dict(kind=2), b"kind"),
                     (dict(kind=-1), b"kind"), (dict(dilate=2), b"dilate"), (dict(dilate=4, dilated=a), b"dilate"), (dict(dilate=11, dilated=a), b"dilate"),
                     (dict(dilate=-1, dilated=a), b"dilate"), (dict(dilate=5), b"null"), (dict(dilate=5, dilated=a, kind=1), b"with labels"),
                     (dict(ws_bytes=8 * tiles - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"), (dict(B=3, ws_bytes=8 * tiles), b"workspace"),
                     (dict(ws=a + 4), b"aligned"), (dict(src=a + 2), b"aligned"), (dict(range=a + 1), b"aligned"),
                     (dict(dilate=3, dilated=a + 2), b"aligned")):
        refused(rng(**kw), b"crd_viz_range", word)
    for kw, word in ((dict(src=None), b"null"), (dict(table=None), b"null"), (dict(out=None), b"null"), (dict(mode=1), b"null"), (dict(mode=2), b"null"),
                     (dict(mode=3), b"null"), (dict(kind=2), b"kind"), (dict(mode=4), b"mode"), (dict(mode=-1), b"mode"),
                     (dict(row=2399), b"row pitch"), (dict(row=0), b"row pitch"), (dict(frame=2400 * 416 - 1), b"frame pitch"),
                     (dict(row=7200, frame=2400 * 416), b"frame pitch"), (dict(range=None, vmin=1.0, vmax=0.5), b"vmin"),
                     (dict(range=None, vmin=nan), b"vmin"), (dict(range=None, vmax=inf), b"vmax"),
                     (dict(mode=2, image=a, alpha=inf), b"alpha"), (dict(mode=2, image=a, beta=nan), b"beta"), (dict(bad=1 << 24), b"bad_rgb"),
                     (dict(bad=-1), b"bad_rgb"), (dict(src=a + 2), b"aligned"), (dict(range=a + 2), b"aligned")):
        refused(draw(**kw), b"crd_viz_draw", word)
    for kw, word in ((dict(logits=None), b"null"), (dict(labels=None), b"null"), (dict(C=0), b"C 0"), (dict(C=257), b"C 257"), (dict(C=-1), b"C -1"),
                     (dict(logits=a + 2), b"aligned")):
        refused(labels(**kw), b"crd_seg_labels", word)


def test_python_interface_refuses_without_a_gpu(built):
    import torch
    from camradepth_amd import viz
    x, lab, img = torch.zeros(2, 5, 7), torch.zeros(2, 5, 7, dtype=torch.uint8), torch.zeros(2, 5, 7, 3, dtype=torch.uint8)
    calls = {"colorize": lambda **kw: viz.colorize(kw.pop("x", x), **kw), "colorize_labels": lambda **kw: viz.colorize_labels(kw.pop("x", lab), **kw),
             "overlay": lambda **kw: viz.overlay(img, kw.pop("x", x), **kw)}
    for name, call in calls.items():
        own = lab if name == "colorize_labels" else x                         # the map of the call's own type
        with pytest.raises(built.CrdError, match="cuda"):                     # host tensors: no CPU fallback
            call()
        with pytest.raises(built.CrdError, match="both vmin and vmax"):
            call(vmin=0.0)
        with pytest.raises(built.CrdError, match="both vmin and vmax"):
            call(vmax=1.0)
        with pytest.raises(built.CrdError, match="vmin <= vmax"):
            call(vmin=1.0, vmax=0.5)
        with pytest.raises(built.CrdError, match="vmin"):
            call(vmin=0.0, vmax=float("nan"))
        with pytest.raises(built.CrdError, match="must be torch"):            # wrong dtypes
            call(x=x.double())
        with pytest.raises(built.CrdError, match="must be torch"):
            call(x=x.long())
        with pytest.raises(built.CrdError, match="shape"):                    # wrong shapes
            call(x=own[0])
        with pytest.raises(built.CrdError, match="shape"):
            call(x=torch.zeros(2, 2, 5, 7, dtype=own.dtype))
        with pytest.raises(built.CrdError, match="shape"):
            call(x=torch.zeros(2, 0, 7, dtype=own.dtype))
    with pytest.raises(built.CrdError, match="float32"):
        viz.colorize(lab)
    with pytest.raises(built.CrdError, match="uint8"):
        viz.colorize_labels(x)
    with pytest.raises(built.CrdError, match="bad_colour"):
        viz.colorize(x, bad_colour=(0, 0, 256))
    with pytest.raises(built.CrdError, match="mode"):
        viz.overlay(img, x, mode="multiply")
    with pytest.raises(built.CrdError, match="image_order"):
        viz.overlay(img, x, image_order="gbr")
    with pytest.raises(built.CrdError, match="alpha"):
        viz.overlay(img, x, mode="blend", alpha=float("inf"))
    for dilate in (0, 2, 11, 2.5, -1):
        with pytest.raises(built.CrdError, match="dilate"):
            viz.radar_overlay(img, x, dilate=dilate)
    for fn, arg in ((viz.radar_overlay, (img, x)), (viz.frame_range, (x,)), (viz.seg_labels, (torch.zeros(2, 21, 5, 7),)), (viz.image_rgb, (img,))):
        with pytest.raises(built.CrdError, match="cuda"):
            fn(*arg)
    with pytest.raises(built.CrdError, match="cmap"):
        viz.table("viridis", "cpu")
    with pytest.raises(built.CrdError, match="cuda"):
        viz.table(torch.zeros(256, 3, dtype=torch.uint8))
    for bad in ((0, 5, 7), (2, 0, 7), (2, 5, -1)):
        with pytest.raises(built.CrdError):
            viz.VizWorkspace(*bad, device="cpu")
    with pytest.raises(built.CrdError, match="image_order"):
        viz.Visualizer(2, 5, 7, image_order="gbr", device="cpu")


def test_workspace_size_query_matches_the_workspace(built):
    import torch
    from camradepth_amd import viz
    assert viz.workspace_bytes(2, 416, 800) == 8 * 2 * 325 and viz.workspace_bytes(1, 1, 1) == 8
    assert viz.workspace_bytes(3, 1, viz.TILE) == 24 and viz.workspace_bytes(3, 1, viz.TILE + 1) == 48
    ws = viz.VizWorkspace(3, 33, 130, device="cpu")       # the buffers are plain tensors: their sizes show without a GPU
    assert ws.partials.dtype == torch.uint8 and ws.partials.numel() == viz.workspace_bytes(3, 33, 130) == 8 * 3 * 5
    assert ws.range.shape == (3, 2) and ws.range.dtype == torch.float32 and ws.dilated.shape == (3, 33, 130) and ws.dilated.dtype == torch.float32
    for name in ("jet", "rainbow"):
        t = viz.table(name, "cpu")
        assert t.shape == (256, 3) and t.dtype == torch.uint8 and bytes(t.flatten().tolist()) == viz.TABLES[name]
    # the C entry refuses one byte less than the query and takes the query itself past the size check (it then fails on the next one)
    L = built.load()
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 15) & ~15
    need = viz.workspace_bytes(3, 33, 130)
    assert L.crd_viz_range(a, 0, 3, 33, 130, 0, None, a, need - 1, a, None) == -1 and b"workspace" in L.crd_last_error()
    assert L.crd_viz_range(a, 0, 3, 33, 130, 0, None, a, need, a + 1, None) == -1 and b"aligned" in L.crd_last_error()
