#!/usr/bin/env python3
"""Launch equality of the weight-gradient routes (tim_amd/csrc/wgrad_plan.h): one timhip_wgrad_group / timhip_wgrad call per
row of the routing table of tests/test_wgrad_plan.py, at the smallest M that reaches each family (2048 / 2051 / 2100 / 1240 /
523), so that two builds of the library can be compared launch by launch:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/wgrad_plan_launches.py      (TIM_AMD_LIB: the other build)
    python tools/wgrad_plan_launches.py --listing OUT > profiles/wgrad_plan_launches_<build>.txt

The listing has one line per weight-gradient kernel in launch order: name, LDS_Block_Size (static LDS only), block, grid in
threads.  The results of the launches are not looked at (tests/test_gpu_kernels.py does that); operands are zeros."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _layer(E, FF):
    return [(E, FF), (FF, E), (E, E), (3 * E, E)]


L4 = _layer(1024, 2048)
# (M, [(Nout, Kout)], knobs, {item: ldy})
GROUPS = [
    (2100, L4, {}, {}),                                                   # loader-wave kernel, 256 tiles
    (2100, L4, {"TIMHIP_WGRAD_LD": "0"}, {}),                             # its 8-wave form
    (2048, L4 + L4, {}, {}),                                              # eight-phase kernel, two phases
    (2048, L4 + L4, {"TIMHIP_WGRAD_P8_PH": "4"}, {}),                     # four phases
    (2048, L4 + L4, {"TIMHIP_WGRAD_P8": "0"}, {}),                        # loader-wave kernel, 512 tiles
    (2048, L4 + L4, {"TIMHIP_WGRAD_P8": "0", "TIMHIP_WGRAD_PP": "0"}, {}),   # split kernel, 1024 tiles, one split
    (2051, L4 + L4, {}, {}),                                              # the ragged instances
    (2051, L4 + L4, {"TIMHIP_WGRAD_P8_PH": "4"}, {}),
    (2048, [(1024, 2048)] * 8, {}, {}),
    (2047, L4 + L4, {}, {}),                                              # M < 2048: split kernel
    (2048, _layer(2048, 4096), {}, {}),                                   # two full rounds of eight-phase tiles
    (2100, _layer(768, 3072), {}, {}),                                    # 768 % 256 != 0: loader-wave kernel, 216 tiles
    (2100, _layer(512, 1024), {}, {}),                                    # 64 tiled tiles < 192: split kernel
    (2100, [(2000, 1000), (1000, 2000), (3000, 1000)], {}, {}),           # ragged n / k tiles
    (1240, [(256, 512), (512, 256), (256, 256), (768, 256)], {}, {}),     # split kernel + reduce
    (523, [(200, 72), (64, 136), (130, 128)], {}, {}),
    (2048, L4 + L4, {}, {5: 1 << 20}),                                    # M * ldy * 2 = 2^32 for one item: split kernel
]
SINGLE = [(1240, 97, 1024), (2100, 300, 1024)]


def run():
    import torch
    from tim_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ru8 = lambda v: (v + 7) // 8 * 8
    for M, shapes, knobs, ldys in GROUPS:
        os.environ.update(knobs)
        L.reload_env()
        keep = []
        arr = (L.TimWgradItem * len(shapes))()
        for i, (N, K) in enumerate(shapes):
            ldy, ldx = ldys.get(i, ru8(N)), ru8(K)
            dY = torch.zeros((M, ldy), dtype=torch.float16, device=dev)
            X = torch.zeros((M, ldx), dtype=torch.float16, device=dev)
            dW = torch.zeros((N, K), device=dev)
            db = torch.zeros((N,), device=dev)
            keep += [dY, X, dW, db]
            arr[i] = L.TimWgradItem(dY.data_ptr(), X.data_ptr(), dW.data_ptr(), db.data_ptr(), ldy, ldx, N, K)
        ws = torch.zeros((lib.timhip_wgrad_group_workspace_bytes(L.PREC_F16, arr, len(shapes), M) + 256,), dtype=torch.uint8, device=dev)
        L.check(lib.timhip_wgrad_group(L.PREC_F16, arr, len(shapes), M, 0, ws.data_ptr(), ws.numel(), None, stream), "timhip_wgrad_group")
        torch.cuda.synchronize()
        for k in knobs:
            del os.environ[k]
    L.reload_env()
    for M, N, K in SINGLE:
        dY = torch.zeros((M, ru8(N)), dtype=torch.float16, device=dev)
        X = torch.zeros((M, K), dtype=torch.float16, device=dev)
        dW, db = torch.zeros((N, K), device=dev), torch.zeros((N,), device=dev)
        ws = torch.zeros((lib.timhip_wgrad_workspace_bytes(L.PREC_F16, N, K, M) + 256,), dtype=torch.uint8, device=dev)
        L.check(lib.timhip_wgrad(L.PREC_F16, dY.data_ptr(), ru8(N), N, X.data_ptr(), K, K, M, dW.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                 ws.numel(), None, stream), "timhip_wgrad")
        torch.cuda.synchronize()


def listing(out_dir):
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows = [r for r in rows if "wgrad" in r["Kernel_Name"] or "slab_reduce" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cols = ("LDS_Block_Size", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z")
    for r in rows:
        print(r["Kernel_Name"], *("%s=%s" % (c, r[c]) for c in cols))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--listing":
        listing(sys.argv[2])
    else:
        run()
