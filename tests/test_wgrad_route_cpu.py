"""The weight-gradient route (csrc/wgrad_route.cpp) sizes every slab: the op-level size functions
and the three networks' workspace plans must answer exactly what the library answered before the
route existed.  A slab is 64 + splits x row floats, so the table pins every split count a size
function can express.  Pure host arithmetic: no GPU needed.

The table (tests/golden/wgrad_route_sizes.json) was recorded from the commit before the route,

    python -m image_denoising_amd._build && python tests/test_wgrad_route_cpu.py --record

and is only re-recorded when a pull request changes a split policy or a tile on purpose."""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "wgrad_route_sizes.json")

NS = (1, 2, 64)
HWS = ((2, 2), (4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (256, 256), (13, 19),
       (7, 40))
CONV3 = ((48, 48), (96, 96), (144, 96), (96, 48), (32, 96), (31, 96))  # (Cin, Cout)
CONV1 = ((96, 96), (96, 1), (96, 3), (96, 4), (48, 48))
DECONV = ((96, 96), (48, 48))
BLOCKED_COUT = (24, 32, 48, 96, 192, 384)
BLOCKED_CIN = (16, 28, 48, 80, 112, 144, 384)
NETS = ("unet", "resnet", "iunet")
NET_SHAPES = ((1, 32, 32), (2, 64, 64), (2, 32, 96), (64, 128, 128), (64, 256, 256),
              (16, 512, 512))
# calls the library refuses with a size of 0; workspace shapes at the networks' limits (the UNet
# refuses all three, the RESNET and ImprovedUNet only the empty batch)
REJECTED_BLOCKED = ((1, 4, 8, 384, 768, 2), (0, 4, 8, 48, 48, 3), (1, 0, 8, 48, 48, 3),
                    (1, 4, 8, 0, 48, 1), (1, 4, 8, 48, 0, 1), (1, 4, 8, 48, 48, 0))
EDGE_NETS = ((2, 48, 64), (0, 64, 64), (1, 16, 16))


def _tables():
    """name -> list of (key, value) in a fixed order, from the loaded library"""
    sys.path.insert(0, ROOT)
    from image_denoising_amd import _lib

    lib = _lib.lib()
    out = {}
    grid = list(itertools.product(NS, HWS))
    for name, shapes, k in (("conv3", CONV3, 3), ("conv1", CONV1, 1)):
        out[name] = [((cin, cout, N, H, W), lib.dn_conv2d_wgrad_slab_size(N, H, W, cin, cout, k))
                     for (cin, cout), (N, (H, W)) in itertools.product(shapes, grid)]
    out["deconv"] = [((cin, cout, N, H, W), lib.dn_deconv2x2_wgrad_slab_size(N, H, W, cin, cout))
                     for (cin, cout), (N, (H, W)) in itertools.product(DECONV, grid)]
    out["blocked"] = [((cin, cout, k, N, H, W),
                       lib.dn_conv2d_wgrad_blocked_slab_size(N, H, W, cin, cout, k))
                      for cout, cin, k, (N, (H, W)) in
                      itertools.product(BLOCKED_COUT, BLOCKED_CIN, (1, 3), grid)]
    out["blocked_rejected"] = [(a, lib.dn_conv2d_wgrad_blocked_slab_size(*a))
                               for a in REJECTED_BLOCKED]

    def workspace(net, C, N, H, W, bwd):
        cfg = _lib.cfg(C, C, 48)
        n = ctypes.c_size_t()
        st = getattr(lib, f"dn_{net}_workspace_size")(ctypes.byref(cfg), N, H, W, bwd,
                                                      ctypes.byref(n))
        return [st, n.value if st == 0 else 0]

    out["workspace"] = [((net, C, N, H, W, bwd), workspace(net, C, N, H, W, bwd))
                        for net, bwd, C, (N, H, W) in
                        itertools.product(NETS, (0, 1), (1, 3), NET_SHAPES)]
    out["workspace_edge"] = [((net, 1, N, H, W, 1), workspace(net, 1, N, H, W, 1))
                             for net, (N, H, W) in itertools.product(NETS, EDGE_NETS)]
    return out


def _load():
    with open(TABLE) as f:
        return json.load(f)


def test_every_size_equals_the_recorded_table():
    want, got = _load(), _tables()
    assert sorted(want) == sorted(got)
    for name in got:
        keys = [list(k) for k, _ in got[name]]
        assert keys == want[name]["keys"], name  # the same cases, none left out
        bad = [(k, v, w) for (k, v), w in zip(got[name], want[name]["values"]) if v != w]
        assert not bad, (name, len(bad), bad[:8])
    assert len(got["blocked"]) == 6 * 7 * 2 * 30 and len(got["workspace"]) == 3 * 2 * 2 * 6
    assert len(got["conv3"]) == 180 and len(got["conv1"]) == 150 and len(got["deconv"]) == 60


def test_rejected_calls_stay_rejected():
    want, got = _load(), _tables()
    assert all(v == 0 for _, v in got["blocked_rejected"]), got["blocked_rejected"]
    was = want["workspace_edge"]["values"]
    assert sum(st != 0 for st, _ in was) == 5
    for (k, (st, n)), (st0, _) in zip(got["workspace_edge"], was):
        assert st0 == 0 or (st != 0 and n == 0), k


def test_slabs_are_whole_rows():
    """64 leading floats, then whole [W ; b] rows; the supported fixed shapes get at least one"""
    got = _tables()
    for (cin, cout, N, H, W), b in got["conv3"]:
        assert b % 4 == 0 and (b // 4 - 64) % (cout * cin * 9 + cout) == 0 and b // 4 > 64
    for (cin, cout, k, N, H, W), b in got["blocked"]:
        assert b % 4 == 0 and (b // 4 - 64) % (cout * cin * k * k + cout) == 0 and b // 4 > 64


if __name__ == "__main__":
    if "--record" in sys.argv:
        t = _tables()
        with open(TABLE, "w") as f:
            json.dump({n: {"keys": [list(k) for k, _ in rows], "values": [v for _, v in rows]}
                       for n, rows in t.items()}, f, separators=(",", ":"))
            f.write("\n")
        print(TABLE, {n: len(rows) for n, rows in t.items()})
