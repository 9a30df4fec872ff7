"""Traversal planning on the GPU (hippt_plan.h): what a render reports of its plan
(HIPPT_INFO_LDS_TOP_BYTES, HIPPT_INFO_CHUNK, HIPPT_INFO_CHAIN_CAP, hipptActiveBvhWidth) is what the
recording of the commit before the planner holds for the same scene, options and call
(tests/golden/traversal_plan_parent.json; tests/test_plan.py replays all of it on the CPU).
HIPPT_INFO_BLOCKS_PER_CU is left out: it follows the compiler's register allocation, not the plan."""
import pytest
import torch  # noqa: F401  before libhippt.so is loaded: both then share one HIP runtime

import hippt
from hippt import scenes
from plan_rows import load_rows

pytestmark = pytest.mark.gpu

W, H, FRAMES, DEPTH = 32, 24, 2, 2
OPTS = ((hippt.OPT_LDS_SCENE, 1), (hippt.OPT_BVH_WIDTH, 0), (hippt.OPT_PATH_MODE, 0), (hippt.OPT_BVH_QUANT, -1),
        (hippt.OPT_CHAIN, -1), (hippt.OPT_COUNT_TRAVERSAL, 0), (hippt.OPT_STACK_CAP, 0), (hippt.OPT_LDS_TOP_NODES, -1),
        (hippt.OPT_CAMERA_POOL, -1), (hippt.OPT_CHUNK, 0))
SCENES = {"cornell34": scenes.cornell34, "cornell_mixed": scenes.cornell_mixed,
          "blob64x34": lambda: scenes.blob_scene(64, 34), "random_scene": scenes.random_scene}
MODES = {"defaults": {}, "PATH_MODE=1": {"pathMode": 1}}  # the recording's names of the options


def row(name, over, pinhole, copy, total):
    """The recorded render launch of scene `name` under the options `over` (the others at their defaults)
    for a call of `total` work items; pinhole: the camera is a pinhole off every coordinate plane."""
    rows = [r for r in load_rows() if r["scene"] == name and r["over"] == over and r["site"] != "launch_query" and
            r["ctx"]["copy"] == copy and r["ctx"]["total"] == total and r["ctx"]["pinhole"] == pinhole]
    assert len(rows) == 1, (name, over, pinhole, copy, total, len(rows))
    return rows[0]


@pytest.fixture()
def pt():
    t = hippt.PathTracer()
    t.setDevices([0])
    t.setRowRange(0, 0)
    for k, v in OPTS:
        t.setOption(k, v)
    yield t
    for k, v in OPTS:
        t.setOption(k, v)
    t.setDevices([])
    hippt.load_library().cudaPathTracerShutdown()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_render_reports_the_recorded_plan(pt, name, mode):
    lib = hippt.load_library()
    info = lambda key: int(lib.hipptGetOption(key))  # noqa: E731
    sc = SCENES[name]()
    pinhole = int(sc.aperture == 0 and all(v != 0 for v in sc.lookfrom))
    pt.uploadMesh(sc)
    if MODES[mode]:
        pt.setOption(hippt.OPT_PATH_MODE, MODES[mode]["pathMode"])
    assert pt.initialize(W, H), pt.lastError()
    tag = name + "|" + mode
    chunk_before = info(hippt.INFO_CHUNK)
    # a blocking call of two frames, then three asynchronous batches of one (chained where the plan allows)
    for copy, total in ((1, W * H * FRAMES), (0, W * H)):
        if copy:
            assert pt.renderFrames(FRAMES, DEPTH), pt.lastError()
        else:
            for _ in range(3):
                assert pt.renderFramesAsync(1, DEPTH), pt.lastError()
            assert pt.synchronize(), pt.lastError()
        r = row(name, MODES[mode], pinhole, copy, total)
        got = (info(hippt.INFO_LDS_TOP_BYTES), info(hippt.INFO_CHAIN_CAP), int(lib.hipptActiveBvhWidth()))
        print(tag, "copy", copy, "site", r["site"], "top bytes / chain cap / width", got, "chunk", info(hippt.INFO_CHUNK),
              "blocks per CU", info(hippt.INFO_BLOCKS_PER_CU))
        if r["site"] == "run_wavefront":
            # HIPPT_INFO_CHUNK and HIPPT_INFO_CHAIN_CAP are the last megakernel batch's: a wavefront leaves them
            assert info(hippt.INFO_CHUNK) == chunk_before
            assert got[0] == r["out"]["topBytes"] and got[2] == (4 if r["out"]["wide"] else 2)
            continue
        assert r["ctx"]["chained"] == (r["site"] == "chain_batch")
        assert got == (r["out"]["topBytes"], r["out"]["chainCap"], 4 if r["out"]["wide"] else 2)
        assert info(hippt.INFO_CHUNK) == r["out"]["chunk"]
