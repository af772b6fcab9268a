"""The refusals of the analysis entry points of include/pivlfn.h, case by case.  A helper, not a test: tests/test_refusal_texts.py replays
the cases below and compares every return code and message with tests/golden/refusal_texts.json.

Per entry point: one base call that passes every argument check, and single-argument perturbations of it that each make one check fail.
Pointers are far-apart integers that are never followed (a refusal comes from the host, before any launch); the few arguments the host
does read (coefficients, tangents, multipliers) are real arrays.  The file also holds, per entry point, one string with one character
per pair of perturbations applied together -- 'a' the message of the first came back, 'b' that of the second, 'x' another refusal (a
message that prints both values), 'n' not refused as a bad argument, '-' both touch the same argument -- which pins the order of the
checks.

Run as a script (`python tests/refusal_cases.py`) it writes the golden file from the library that is built.  That is done only by a
pull request that means to change a refusal; the file then has to reproduce from that pull request's sources byte for byte.  It needs
no GPU and must not see one: a call that is not refused would be launched on made-up pointers.
"""
import ctypes
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "refusal_texts.json")
INF, NAN = math.inf, math.nan
BIG = 46341                      # BIG * BIG >= 2^31


class Ref:
    """The value of another argument of the same call, plus an offset: an output moved onto an input, a workspace one byte short."""
    def __init__(self, name, delta=0):
        self.name, self.delta = name, delta


class Need:
    """The bytes a workspace query of the library returns for the base call's sizes."""
    def __init__(self, query, *names):
        self.query, self.names = query, names


def null(*names):
    return [(f"{n}=null", {n: None}) for n in names]


def vals(name, *values):
    return [(f"{name}={v!r}", {name: v}) for v in values]


def both(label=None, **kw):
    return [(label or ",".join(f"{k}={v!r}" for k, v in kw.items()), kw)]


def onto(outs, ins):
    """Every output moved onto every input."""
    return [(f"{o}@{i}", {o: Ref(i)}) for o in outs for i in ins]


def among(outs):
    """Every output moved onto every other output."""
    return [(f"{o}@{p}", {o: Ref(p)}) for k, o in enumerate(outs) for p in outs[k + 1:]]


def off(name, delta):
    return [(f"{name}{delta:+d}", {name: Ref(name, delta)})]


def shape3(b="B", h="H", w="W", top=65536):
    """The shape triple: a zero, a negative and a too-large size."""
    out = vals(b, 0) + vals(h, -1) + vals(w, 0) + both(**{h: BIG, w: BIG})
    return out + (vals(b, top) if top else [])


_F2 = (ctypes.c_float * 2)(2.0, 0.5)
_COEFF = (ctypes.c_float * 48)(*[0.25 * (k % 7 + 1) for k in range(48)])
_TAN = (ctypes.c_double * 4)(-0.5, 0.5, 0.1, 0.1)
_TAN_INF = (ctypes.c_double * 4)(-0.5, INF, 0.1, 0.1)
_TAN_EQ = (ctypes.c_double * 4)(0.5, 0.5, 0.1, 0.1)
_A = (ctypes.c_double * 24)(*[0.5 + 0.125 * k for k in range(24)])
_A_NAN = (ctypes.c_double * 24)(*[NAN if k == 7 else 1.0 for k in range(24)])
HOST = {"F2": _F2, "COEFF": _COEFF, "TAN": _TAN, "TAN_INF": _TAN_INF, "TAN_EQ": _TAN_EQ, "A": _A, "A_NAN": _A_NAN}


class Host:
    """A real host array of HOST, by name (so that a label can print it)."""
    def __init__(self, key):
        self.key = key

    def __repr__(self):
        return self.key


# name -> (argument names in call order without the stream, base values of the non-pointer arguments, perturbations).  An argument
# without a base value is a device pointer: it gets the next far-apart address.
ENTRY_POINTS = {
    "pivlfn_stereo_2d3c": (
        "flow out B h w H W mul coeff scale tangents",
        dict(B=2, h=8, w=8, H=16, W=16, mul=Host("F2"), coeff=Host("COEFF"), scale=None, tangents=Host("TAN")),
        # mul and scale may be null
        null("flow", "out", "coeff", "tangents") + vals("B", 0, 65536) + vals("h", 0) + vals("w", -1) + vals("H", 0) + vals("W", 0)
        + both(H=BIG, W=BIG) + both(h=BIG, w=BIG) + vals("tangents", Host("TAN_INF"), Host("TAN_EQ"))),
    "pivlfn_flow_fields": (
        "flow out B H W calib kind out_f64", dict(B=2, H=8, W=8, calib=1.0, kind=0, out_f64=0),
        null("flow", "out") + shape3() + vals("calib", 0.0, INF, NAN, 1e308) + vals("kind", -1, 2) + vals("out_f64", 2)),
    "pivlfn_flow_stats_accumulate": (
        "flow acc B H W calib", dict(B=2, H=8, W=8, calib=1.0),
        # B = 65536 is not refused: the frames are a loop of the kernel, not a grid dimension
        null("flow", "acc") + shape3(top=0) + vals("calib", 0.0, INF, NAN, 1e308)),
    "pivlfn_flow_validate": (
        "flow out flag resid B H W radius spacing eps thresh mode", dict(B=2, H=8, W=8, radius=1, spacing=1, eps=0.1, thresh=2.0, mode=2),
        # resid may be null; out is compared with flow by address only
        null("flow", "flag", "out") + onto(["out"], ["flow"]) + vals("mode", -1, 3) + shape3() + vals("radius", 0, 3)
        + vals("spacing", 0, 32768) + vals("eps", -1.0, INF, NAN) + vals("thresh", 0.0, INF, NAN)),
    "pivlfn_flow_stats_accumulate_masked": (
        "flow flag acc cnt B H W calib", dict(B=2, H=8, W=8, calib=1.0),
        null("flow", "flag", "acc", "cnt") + shape3(top=0) + vals("calib", 0.0, INF, NAN, 1e308)),
    "pivlfn_frames_preprocess": (
        "frames bg out n H W k floor", dict(n=2, H=8, W=8, k=3, floor=10),
        # bg may be null
        null("frames", "out") + vals("n", 0, 65536) + vals("H", 0) + vals("W", -1) + both(H=26755, W=26755) + vals("k", 1, 2, 4, 33)
        + vals("floor", 0, 256) + onto(["out"], ["frames", "bg"])),
    "pivlfn_frames_background_min": (
        "frames bg n H W", dict(n=2, H=8, W=8),
        null("frames", "bg") + vals("n", 0) + vals("H", 0) + vals("W", -1) + both(H=26755, W=26755) + onto(["bg"], ["frames"])),
    "pivlfn_flow_errors": (
        "flow truth mask B H W k div_flow sums err_map ws ws_bytes",
        dict(B=2, H=64, W=64, k=1, div_flow=20.0, ws_bytes=Need("pivlfn_flow_errors_workspace_bytes", "B", "H", "W")),
        # mask and err_map may be null; the op checks no aliasing
        null("flow", "truth", "sums", "ws") + shape3() + vals("div_flow", INF, NAN) + off("ws", 4) + off("ws_bytes", -1) + vals("k", -1, 6)
        + vals("H", 63)),
    "pivlfn_level_errors": (
        "levels lowest_level truth mask B H W div_flow sums ws ws_bytes",
        dict(lowest_level=2, B=2, H=64, W=64, div_flow=20.0, ws_bytes=Need("pivlfn_flow_errors_workspace_bytes", "B", "H", "W")),
        null("levels", "truth", "sums", "ws") + shape3() + vals("div_flow", INF, NAN) + off("ws", 4) + off("ws_bytes", -1)
        + vals("lowest_level", 0, 7) + vals("W", 48)),
    "pivlfn_error_stats_accumulate": (
        "flow truth mask acc B H W", dict(B=2, H=8, W=8),
        null("flow", "truth", "acc") + shape3(top=0)),
    "pivlfn_flow_maxrad": ("flow mask maxrad B H W", dict(B=2, H=8, W=8), null("flow", "maxrad") + shape3()),
    "pivlfn_flow_to_color": (
        "flow norm mask out B H W wheel order", dict(B=2, H=8, W=8, wheel=0, order=1),
        null("flow", "norm", "out") + shape3() + vals("wheel", -1, 2) + vals("order", 2)),
    "pivlfn_field_absmax": (
        "field is_f64 mask absmax B H W", dict(is_f64=0, B=2, H=8, W=8), null("field", "absmax") + shape3() + vals("is_f64", -1, 2)),
    "pivlfn_scalar_to_color": (
        "field is_f64 mask lut out B H W vmin vmax bad_rgb", dict(is_f64=1, B=2, H=8, W=8, vmin=0.0, vmax=1.0, bad_rgb=0xFF00FF),
        null("field", "lut", "out") + shape3() + vals("is_f64", 2) + vals("vmin", INF, 1.0) + vals("vmax", NAN, 5e-324)
        + vals("bad_rgb", -1, 0x1000000)),
    "pivlfn_flow_decimate": (
        "flow mask mean count B H W cell", dict(B=2, H=8, W=8, cell=4),
        null("flow", "mean", "count") + shape3() + vals("cell", 0, 32769)),
    "pivlfn_match_quality": (
        "img1 img2 C flow mask quality flag B H W radius min_count floor ws ws_bytes",
        dict(C=1, B=2, H=8, W=8, radius=2, min_count=13, floor=1 / 255,
             ws_bytes=Need("pivlfn_match_quality_workspace_bytes", "B", "H", "W", "radius")),
        null("img1", "img2", "flow", "quality", "flag", "ws") + vals("C", 0, 2) + shape3() + vals("radius", 0, 16) + vals("min_count", 1, 26)
        + vals("floor", -0.5, INF, NAN) + off("ws", 4) + off("ws_bytes", -1)
        + onto(["quality", "flag"], ["img1", "img2", "flow", "mask", "ws"]) + among(["quality", "flag"])),
    "pivlfn_vortex_gamma": (
        "flow mask gamma flag B H W radius spacing min_count ws ws_bytes",
        dict(B=2, H=8, W=8, radius=2, spacing=1, min_count=12,
             ws_bytes=Need("pivlfn_vortex_gamma_workspace_bytes", "B", "H", "W", "radius", "spacing")),
        null("flow", "gamma", "flag", "ws") + shape3() + vals("radius", 0, 16) + vals("spacing", 0, 17) + vals("min_count", 0, 25)
        + off("ws", 4) + off("ws_bytes", -1) + onto(["gamma", "flag"], ["flow", "mask", "ws"]) + among(["gamma", "flag"])),
    "pivlfn_flowmap_advect": (
        "flows mask B H W pos flag N backward iters trace", dict(B=2, H=8, W=8, N=10, backward=0, iters=4),
        # mask and trace may be null
        vals("H", 1) + vals("W", 1) + both(H=BIG, W=BIG) + vals("B", -1) + vals("N", -1) + vals("backward", -1, 2) + vals("iters", 0, 33)
        + null("flows", "pos", "flag") + onto(["pos", "flag", "trace"], ["flows", "mask"]) + among(["pos", "flag", "trace"])),
    "pivlfn_flowmap_seed": (
        "pos flag h w spacing", dict(h=6, w=7, spacing=4),
        vals("h", 0) + vals("w", -1) + both(h=BIG, w=BIG) + vals("spacing", 0, 32769) + both(h=65537, spacing=32768) + null("pos", "flag")
        + among(["pos", "flag"])),
    "pivlfn_flowmap_ftle": (
        "pos flag h w spacing stretch oflag", dict(h=6, w=7, spacing=4),
        vals("h", 0) + vals("w", -1) + both(h=BIG, w=BIG) + vals("spacing", 0, 32769) + both(w=65537, spacing=32768)
        + null("pos", "flag", "stretch", "oflag") + onto(["stretch", "oflag"], ["pos", "flag"]) + among(["stretch", "oflag"])),
    "pivlfn_particles_displace": (
        "pos flow mask H W N method flag out", dict(H=8, W=8, N=10, method=1),
        vals("H", 1) + vals("W", 0) + both(H=BIG, W=BIG) + vals("N", -1) + vals("method", -1, 2) + null("pos", "flow", "flag", "out")
        + onto(["out", "flag"], ["pos", "flow", "mask"]) + among(["out", "flag"])),
    "pivlfn_particles_render": (
        "pos diam amp flag B N H W radius intensity image workspace workspace_bytes",
        dict(B=2, N=10, H=16, W=16, radius=2, workspace_bytes=Need("pivlfn_particles_render_workspace_bytes", "B", "N", "H", "W", "radius")),
        # flag may be null
        vals("H", 0) + vals("W", -1) + vals("H", 2147483647) + both(H=BIG, W=BIG) + vals("B", -1) + vals("N", -1) + vals("radius", 0, 9)
        + null("intensity", "image", "workspace", "pos", "diam", "amp") + off("workspace", 4) + off("workspace_bytes", -1)
        + onto(["intensity", "image", "workspace"], ["pos", "diam", "amp", "flag"]) + among(["intensity", "image", "workspace"])),
    "pivlfn_snapshot_gram": (
        "X n P ldx G ws ws_bytes", dict(n=4, P=100, ldx=100, ws_bytes=Need("pivlfn_snapshot_gram_workspace_bytes", "n", "P")),
        null("X", "G", "ws") + vals("n", 0, 4097) + vals("P", 0, 1 << 31) + vals("ldx", 99) + off("ws", 4) + off("ws_bytes", -1)),
    "pivlfn_snapshot_project": (
        "X n P ldx Wt K out", dict(n=4, P=100, ldx=100, K=3),
        null("X", "Wt", "out") + vals("n", 0, 4097) + vals("P", 0, 1 << 31) + vals("ldx", 99) + vals("K", 0, 65)),
    "pivlfn_twopoint_accumulate": (
        "flow mask mean acc B H W max_sep step", dict(B=2, H=8, W=8, max_sep=4, step=1),
        # mask and mean may be null
        vals("H", 0) + vals("W", -1) + vals("B", -1) + both(H=BIG, W=BIG) + vals("W", 16385) + vals("max_sep", -1, 256) + vals("step", 0, 17)
        + null("flow", "acc") + onto(["acc"], ["flow", "mask", "mean"])),
    "pivlfn_spectrum_accumulate": (
        "X L first N ldx basis K acc count", dict(L=16, first=0, N=10, ldx=20, K=4),
        # the op checks no aliasing
        null("X", "basis", "acc", "count") + vals("L", 1, 1025) + vals("first", -1, 16) + vals("K", 0, 514) + vals("N", 0, 1 << 30)
        + vals("ldx", 19)),
    "pivlfn_pressure_gradient": (
        "flows B h w s nu g valid", dict(B=3, h=8, w=8, s=1.0, nu=0.0),
        vals("B", 2) + vals("h", 0) + vals("w", -1) + both(h=BIG, w=BIG) + vals("s", 0.0, INF, NAN) + vals("nu", INF, NAN)
        + null("flows", "g", "valid") + onto(["g", "valid"], ["flows"]) + onto(["valid"], ["g"])),
    "pivlfn_pressure_setup": (
        "g valid F h w s ws ws_bytes", dict(F=1, h=8, w=8, s=1.0, ws_bytes=Need("pivlfn_pressure_workspace_bytes", "F", "h", "w")),
        vals("F", 0) + vals("h", 0) + vals("w", -1) + both(h=BIG, w=BIG) + vals("s", 0.0, INF, NAN) + null("g", "valid", "ws") + off("ws", 4)
        + off("ws_bytes", -1) + onto(["ws"], ["g", "valid"])),
    "pivlfn_pressure_cg": (
        "ws ws_bytes F h w tol iters", dict(F=1, h=8, w=8, tol=1e-6, iters=5, ws_bytes=Need("pivlfn_pressure_workspace_bytes", "F", "h", "w")),
        vals("F", 0) + vals("h", 0) + vals("w", -1) + both(h=BIG, w=BIG) + vals("tol", 0.0, INF, NAN) + vals("iters", -1) + null("ws")
        + off("ws", 4) + off("ws_bytes", -1)),
    "pivlfn_pressure_read": (
        "ws ws_bytes F h w p flag status", dict(F=1, h=8, w=8, ws_bytes=Need("pivlfn_pressure_workspace_bytes", "F", "h", "w")),
        vals("F", 0) + vals("h", 0) + vals("w", -1) + both(h=BIG, w=BIG) + null("p", "flag", "status", "ws") + off("ws", 4)
        + off("ws_bytes", -1) + onto(["p", "flag", "status"], ["ws"]) + among(["p", "flag", "status"])),
    "pivlfn_template_match": (
        "images templ r B H W th tw ws ws_bytes",
        dict(B=2, H=32, W=32, th=5, tw=5, ws_bytes=Need("pivlfn_template_match_workspace_bytes", "th", "tw")),
        # the op checks no aliasing
        null("images", "templ", "r", "ws") + shape3() + vals("th", 0, 4) + vals("tw", -1, 6) + both(th=257, tw=257) + off("ws", 2)
        + off("ws_bytes", -1)),
    "pivlfn_target_points": (
        "r B H W threshold cap labels count rec ws ws_bytes",
        dict(B=2, H=32, W=32, threshold=0.5, cap=100, ws_bytes=Need("pivlfn_target_points_workspace_bytes", "B", "H", "W")),
        null("r", "labels", "count", "rec", "ws") + shape3() + vals("cap", 0, (1 << 24) + 1) + vals("threshold", NAN) + off("ws", 2)
        + off("rec", 4) + off("ws_bytes", -1)),
    "pivlfn_dewarp_frames": (
        "frames out is_f32 B H W A x0 y0 mode fill", dict(is_f32=0, B=2, H=8, W=8, A=Host("A"), x0=0.0, y0=0.0, mode=1, fill=0.0),
        # out is compared with frames by address only
        null("frames", "out", "A") + onto(["out"], ["frames"]) + vals("is_f32", -1, 2) + shape3() + vals("mode", -1, 2) + vals("x0", INF)
        + vals("y0", NAN) + vals("A", Host("A_NAN")) + vals("fill", -1.0, 0.5, 256.0, NAN) + both(is_f32=1, fill=1e39)),
    "pivlfn_flow_uncertainty": (
        "img1 img2 C flow mask unc flag B H W radius lag min_count floor ws ws_bytes",
        dict(C=3, B=2, H=8, W=8, radius=2, lag=1, min_count=13, floor=1 / 255,
             ws_bytes=Need("pivlfn_flow_uncertainty_workspace_bytes", "B", "H", "W", "radius", "lag")),
        null("img1", "img2", "flow", "unc", "flag", "ws") + vals("C", 0, 2) + shape3() + vals("radius", 0, 16) + vals("lag", -1, 5)
        + vals("min_count", 1, 26) + vals("floor", -0.5, INF, NAN) + off("ws", 4) + off("ws_bytes", -1)
        + onto(["unc", "flag"], ["img1", "img2", "flow", "mask", "ws"]) + among(["unc", "flag"])),
    "pivlfn_uncertainty_accumulate": (
        "unc flag sums B H W", dict(B=2, H=8, W=8),
        null("unc", "flag", "sums") + shape3(top=0) + off("sums", 4) + onto(["sums"], ["unc", "flag"])),
}


def gpu_visible():
    import torch
    return torch.cuda.is_available()


def _library():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "piv_liteflownet-pytorch_amd"))
    from pivlfn import _lib
    return _lib.load()


def base_call(lib, name):
    """The base arguments of `name` as a dict in call order: far-apart addresses for the device pointers, the workspace sizes asked of
    the library."""
    names, base, _ = ENTRY_POINTS[name]
    args, k = {}, 0
    for n in names.split():
        if n in base:
            args[n] = base[n]
        else:
            args[n] = (1 << 20) + (k << 32)
            k += 1
    for n, v in args.items():
        if isinstance(v, Need):
            args[n] = getattr(lib, v.query)(*(args[m] for m in v.names))
            assert args[n] > 0, (name, v.query)
    return args


def call(lib, name, base, *changes):
    """(return code, message) of `name` with the changes applied to the base arguments."""
    args = dict(base)
    for change in changes:
        for n, v in change.items():
            args[n] = base[v.name] + v.delta if isinstance(v, Ref) else v
    values = [HOST[v.key] if isinstance(v, Host) else v for v in args.values()]
    rc = getattr(lib, name)(*values, None)
    return rc, lib.pivlfn_last_error().decode() if rc else ""


def record(lib, name):
    """{"cases": {label: [code, message]}, "order": one character per pair of perturbations} of one entry point."""
    base = base_call(lib, name)
    cases = ENTRY_POINTS[name][2]
    labels = [label for label, _ in cases]
    assert len(set(labels)) == len(labels), (name, labels)
    single = {label: list(call(lib, name, base, change)) for label, change in cases}
    order = []
    for i, (la, a) in enumerate(cases):
        for lb, b in cases[i + 1:]:
            if set(a) & set(b):
                order.append("-")
                continue
            rc, msg = call(lib, name, base, a, b)
            order.append("n" if rc != 1 else "a" if msg == single[la][1] else "b" if msg == single[lb][1] else "x")
    return {"cases": single, "order": "".join(order)}


def record_all(lib):
    return {name: record(lib, name) for name in ENTRY_POINTS}


def main():
    assert not gpu_visible(), "a GPU is visible: a call that is not refused would be launched on made-up pointers"
    lib = _library()
    out = record_all(lib)
    for name, entry in out.items():
        rc, _ = call(lib, name, base_call(lib, name))
        assert rc != 1, f"{name}: the base call is refused: {lib.pivlfn_last_error().decode()}"
        for label, (code, msg) in entry["cases"].items():
            assert code == 1, f"{name} {label}: not refused as a bad argument (code {code}, {msg!r}): drop the case, with a comment"
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{GOLDEN}: {sum(len(e['cases']) for e in out.values())} refusals of {len(out)} entry points")


if __name__ == "__main__":
    main()
