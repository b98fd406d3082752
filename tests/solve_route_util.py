"""What tests/test_solve_route_host.py and tests/test_gpu_solve_route.py share: the line grammar of
tests/host/solve_route_harness.cpp (one request per line -> the fields of the SolveRoute that route_solve returns) and a
restatement, from those fields, of the kernel names the library's launchers note -- written from the names as
profiles/launch_layer_routing_table.md and include/mrs_tg.h spell them, not from the launchers' code."""
from tests import host_harness as hh

FIXED, CLOSING = 0, 1
FORCE_ROWS, FORCE_TILE = 1, 2


def build(tmp_path, sanitize=False):
    return hh.build("solve_route_harness.cpp", tmp_path, sanitize=sanitize)


def request(n, S, uniform=None, d=4, fused=1, store=1, group=0, wp=0, shared=0, slots=0, cus=256, stage=FIXED, scale=0, maxima=0,
            sampling=0, force=0):
    """one input line; uniform: uniform_S (default: every path has S segments; 0: a ragged batch whose longest path has S)"""
    v = [n, S, S if uniform is None else uniform, d, fused, store, group, wp, shared, slots, cus, stage, scale, maxima, sampling, force]
    return " ".join(str(int(x)) for x in v) + "\n"


def closing_requests(n, S, uniform=None, general=False, samples=True, **kw):
    """the two closing solves of a Mellinger pipeline as it asks for them: the trajectory of the last evaluated point, then the
    solve at the scaled times -- with the maxima, the scaling and the sampling where its launch can take them"""
    take = 0 if general else 1
    return [request(n, S, uniform, **kw),
            request(n, S, uniform, stage=CLOSING, scale=take, maxima=take, sampling=int(samples and not general), **kw)]


def parse(line):
    r = {}
    for item in line.split():
        k, v = item.split("=")
        r[k] = v if k == "family" else int(v)
    return r


def routes(exe, lines, env=None):
    return [parse(x) for x in hh.run(exe, lines, len(lines), env=env)]


def _b(x):
    return "true" if x else "false"


def kernel_name(r, spell_instantiations=False):
    """the name in the kernel trace of the launch a route describes"""
    f, grouped = r["family"], r["group"] > 0
    if f == "rows":
        return "solve_rows_group_kernel" if grouped else "solve_rows_kernel<%d>" % r["with_tail"]
    if f == "rows_pipeline":
        return "solve_rows_pipeline_kernel"
    if f == "tile":
        return "solve_tile_kernel<%s>" % _b(r["fused"])
    if f == "lane":   # dimensions per lane, then fused; the parentheses are part of the name
        return "(solve_linear_kernel<%d, %s>)" % (4 // r["lanes_per_path"], _b(r["fused"]))
    if f == "duo":
        if grouped:   # the lean instantiation goes by its family's name unless MRS_TG_TRACE_INSTANTIATIONS asks
            return "solve_duo_group_kernel<%s%s>" % (_b(r["wp"]), ", true" if r["lean"] and spell_instantiations else "")
        return "solve_duo_kernel<%s>" % _b(r["wp"])
    if f == "quad":
        return "solve_quad%s_kernel<%s%s>" % ("_group" if grouped else "", _b(r["wp"]), ", true" if r["ends"] else "")
    raise AssertionError(r)


def closing_names(first, final):
    """the solve_* launches that close a pipeline: one launch where the final solve takes the maxima into it, else both"""
    return [kernel_name(final)] if final["maxima_in_launch"] else [kernel_name(first), kernel_name(final)]
