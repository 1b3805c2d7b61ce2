"""CPU: the C ABI of the point-cloud back end without a GPU.  tests/test_abi.py parses the header against the library and the binding
and so covers the two new declarations; here both entries refuse bad arguments before any GPU call, with the documented status and a
crd_last_error text, and the Python interface refuses host tensors.  stride, the workspace and rgb are arguments of crd_point_cloud
alone."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crd_depth_unproject", "crd_point_cloud")


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
        assert not [a for a in args.split(",") if "double" in a and "*" not in a], name       # fp64 through memory or as bit patterns
    assert L.crd_version() == 13                                                               # no struct, no changed signature
    from camradepth_amd import cloud
    assert cloud.TILE == int(re.search(r"#define\s+CRD_CLOUD_TILE\s+(\d+)", h).group(1))


def test_invalid_arguments_are_reported_without_a_gpu(built):
    L = built.load()
    buf = ctypes.create_string_buffer(256)               # any aligned non-NULL host address: a refused call launches nothing, reads none of it
    a = (ctypes.addressof(buf) + 15) & ~15
    bits = built.f64_bits
    inf = float("inf")

    def lead(v):
        return (v["depth"], v["B"], v["im_h"], v["im_w"], v["s"], v["cut"], v["K"], v["k_stride"], v["T"], v["t_stride"], v["encoding"],
                bits(v["max_depth"]), bits(v["min_range"]), bits(v["max_range"]), 0, v["mask"], v["labels"], v["keep"])

    base = dict(depth=a, B=2, im_h=900, im_w=1600, s=2, cut=34, K=a, k_stride=0, T=None, t_stride=0, encoding=0, max_depth=100.0,
                min_range=0.0, max_range=inf, mask=None, labels=None, keep=None)

    def unproject(**kw):
        v = dict(base, points=a, valid=a)
        v.update(kw)
        return L.crd_depth_unproject(*lead(v), v["points"], v["valid"], None)

    def cloud(**kw):
        v = dict(base, stride=1, image=None, ws=a, ws_bytes=1 << 40, xyz=a, rgb=None, label=None, pixel=None, off=a)
        v.update(kw)
        return L.crd_point_cloud(*lead(v), v["stride"], v["image"], v["ws"], v["ws_bytes"], v["xyz"], v["rgb"], v["label"], v["pixel"],
                                 v["off"], None)

    def refused(rc, name, word):
        msg = L.crd_last_error()
        assert rc == -1 and name in msg and word in msg, (rc, msg)
        with pytest.raises(built.CrdError):
            built.check(rc, name.decode())

    shared = ((dict(depth=None), b"null"), (dict(K=None), b"null"), (dict(B=0), b"bad argument"), (dict(B=-3), b"bad argument"),
              (dict(k_stride=3), b"k_stride"), (dict(k_stride=-9), b"k_stride"), (dict(t_stride=9), b"t_stride"),
              (dict(T=a, t_stride=3), b"t_stride"), (dict(encoding=2), b"encoding"), (dict(encoding=-1), b"encoding"),
              (dict(labels=a), b"labels without keep"), (dict(cut=-1), b"y_cutoff"), (dict(cut=450), b"y_cutoff"),
              (dict(s=0), b"downsample_scale"), (dict(s=901), b"downsample_scale"), (dict(im_w=0), b"bad argument"),
              (dict(max_depth=0.0), b"max_depth"), (dict(max_depth=inf), b"max_depth"), (dict(max_depth=float("nan")), b"max_depth"),
              (dict(min_range=float("nan")), b"min_range"), (dict(max_range=float("nan")), b"max_range"),
              (dict(depth=a + 4), b"aligned"), (dict(mask=a + 2), b"aligned"), (dict(labels=a + 1, keep=a), b"aligned"))
    for kw, word in shared:
        refused(unproject(**kw), b"crd_depth_unproject", word)
        refused(cloud(**kw), b"crd_point_cloud", word)
    for kw, word in ((dict(points=None), b"null"), (dict(valid=None), b"null"), (dict(points=a + 8), b"aligned"),
                     (dict(valid=a + 2), b"aligned")):
        refused(unproject(**kw), b"crd_depth_unproject", word)
    tiles = 2 * 325                                       # 416 x 800 candidates per frame in tiles of 1024
    for kw, word in ((dict(stride=0), b"stride"), (dict(stride=-2), b"stride"), (dict(ws_bytes=4 * tiles - 1), b"workspace"),
                     (dict(ws_bytes=0), b"workspace"), (dict(stride=2, ws_bytes=4 * 2 * 82 - 1), b"workspace"),
                     (dict(rgb=a), b"rgb without image"), (dict(label=a), b"label without labels"), (dict(xyz=None), b"null"),
                     (dict(off=None), b"null"), (dict(ws=None), b"null"), (dict(ws=a + 2), b"aligned")):
        refused(cloud(**kw), b"crd_point_cloud", word)


def test_python_interface_refuses_host_tensors_without_a_gpu(built):
    import torch
    from camradepth_amd import cloud
    K = torch.eye(3, dtype=torch.float64)
    for fn in (cloud.unproject_depth, cloud.point_cloud):
        with pytest.raises(built.CrdError, match="cuda") as refusal:
            fn(torch.zeros(1, 416, 800), K)
        assert "radar" not in str(refusal.value)
        with pytest.raises(built.CrdError, match="encoding"):
            fn(torch.zeros(1, 416, 800), K, encoding="disparity")
    with pytest.raises(built.CrdError, match="stride"):
        cloud.point_cloud(torch.zeros(1, 416, 800), K, stride=0)
    assert cloud.candidates(416, 800) == 332800 and cloud.candidates(17, 32, 3) == 6 * 11
    assert cloud.workspace_bytes(2, 416, 800) == 4 * 2 * 325 and cloud.workspace_bytes(2, 416, 800, 2) == 4 * 2 * 82
    assert cloud.workspace_bytes(3, 1, cloud.TILE) == 12 and cloud.workspace_bytes(3, 1, cloud.TILE + 1) == 24
    table = cloud.keep_table({0, 3, 255}, device="cpu")
    assert table.dtype == torch.uint8 and table.shape == (256,) and table.nonzero().flatten().tolist() == [0, 3, 255]
    with pytest.raises(built.CrdError):
        cloud.keep_table([256], device="cpu")
