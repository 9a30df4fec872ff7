"""Reader of tests/golden/traversal_plan_parent.json (the launch scalars recorded before the traversal
planner existed; tests/test_plan.py, tests/test_gpu_plan.py): every row as a dict of site, scene, facts,
knobs (all of them), over (the options off their defaults), limits, ctx and out."""
import functools
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traversal_plan_parent.json")
RENDER_CTX, QUERY_CTX = 6, 4  # leading call-context columns of render_columns / query_columns


@functools.lru_cache(maxsize=None)
def load_rows():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["recorded_from"] and doc["note"]
    rows = []
    for site, scene, half, over, *vals in doc["rows"]:
        query = site == "launch_query"
        cols = doc["query_columns" if query else "render_columns"]
        assert len(vals) == len(cols), (site, len(vals))
        n = QUERY_CTX if query else RENDER_CTX
        name = doc["scene_names"][scene]
        rows.append({"site": site, "scene": name, "facts": dict(doc["scenes"][name], halfTree=half),
                     "knobs": dict(doc["knob_defaults"], **over), "over": over, "limits": doc["limits"],
                     "ctx": dict(zip(cols[:n], vals[:n])), "out": dict(zip(cols[n:], vals[n:]))})
    return rows
