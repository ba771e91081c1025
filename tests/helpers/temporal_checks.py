"""Stage checks of the temporal branch, shared by tests/test_gpu_temporal_stages.py (the GPU's taps against the float64 stage references) and
tests/test_temporal_stage_checks_cpu.py (the same checks fed the fp32 restatement, which must pass, and mutated references, which must fail).

One check per GPU launch: the launch's output against the float64 stage function of oracle/grnet_oracle.py on the launch's OWN fp32 input.  The walkers
below (ts_walk, gru_walk, fc_walk) go through a module launch by launch and yield (stage, got, reference); where the inputs come from is the caller's: the
taps of a GPU call (TapSource) or the fp32 restatement's own outputs (HostSource, which also serves tools/temporal_stage_floors.py).

BARS.  Not taken from the kernels: FLOORS holds, per stage, metric and size class, the error of the plain fp32 restatement (the oracle's stage function
outside float64(), numpy / BLAS float32) against the float64 stage reference on the same fp32 input, measured on a CPU by tools/temporal_stage_floors.py --
the rounding floor of an honest fp32 implementation.  The bar is 8 x that floor (a different summation order: 4-wide MFMA chains, key blocks, fixed-order
part merges; v_exp_f32 / v_rcp_f32 against libm), never above the module-level bar already in force (5e-5 attention block, 1e-4 GRU, 3e-5 corrector).

Metrics: "t" = rel_err of the tensor, max |a - b| / max |b|; "r" = the same per vector of the last axis, worst vector (a query row of one head for the
attention stages): a fault confined to one row whose values are small against the tensor's largest does not hide behind that largest value.
"""
import numpy as np

MODULE_BAR = {"ts": 5e-5, "gru": 1e-4, "fc": 3e-5}
FLOOR_FACTOR = 8.0

# size classes: the attention block by frames per clip, the GRU by steps; floors are the largest seen over the class's sizes
TS_CLASSES = (("S", 64, ((4, 64), (1, 16), (1, 1))), ("M", 1100, ((1, 383), (1, 384), (2, 1100))), ("L", 10000, ((1, 7200), (1, 10000))),
              ("XL", 32768, ((1, 17000), (1, 32768))))
GRU_CLASSES = (("S", 64, ((1, 16), (4, 64), (16, 9))), ("M", 2000, ((3, 257), (1, 2000))), ("L", 10000, ((1, 10000),)))
FC_CLASSES = (("S", 64, ((1, 16), (4, 64))), ("L", 10000, ((1, 10000),)))


def size_class(module, n):
    for name, top, _ in {"ts": TS_CLASSES, "gru": GRU_CLASSES, "fc": FC_CLASSES}[module]:
        if n <= top:
            return name
    raise ValueError(f"no size class for {module} at {n}")


# stage -> metrics checked.  ts.* stages inside the corrector are the attention block's and use its floors.
ROW_STAGES = ("ts.x_t", "ts.part_o", "ts.x_s", "ts.x_t_gated", "ts.x_s_gated")

# FLOORS[module class][stage][metric]: measured by `python tools/temporal_stage_floors.py` (8 threads, numpy + OpenBLAS float32 against float64).
# BEGIN FLOORS (generated)
FLOORS = {'ts:S': {'ts.qkv_t': {'t': 5.505042754816013e-07},
          'ts.qkv_s': {'t': 5.780675459567592e-07},
          'ts.x_t': {'t': 7.35951330060549e-07, 'r': 1.29533579881718e-06},
          'ts.x_s': {'t': 5.712765092098232e-07, 'r': 8.479966809269769e-07},
          'ts.mean': {'t': 3.657956259779589e-07},
          'ts.logits': {'t': 7.018219436260903e-07},
          'ts.x_t_gated': {'t': 1.125155597545435e-07, 'r': 1.5558279860155553e-07},
          'ts.x_s_gated': {'t': 1.0922275874466194e-07, 'r': 1.542941729234838e-07},
          'ts.y_t': {'t': 7.514793055253309e-07},
          'ts.y_s': {'t': 6.37509216581357e-07},
          'ts.x1': {'t': 2.1110481238882043e-07},
          'ts.out': {'t': 2.564591014668516e-07}},
 'ts:M': {'ts.qkv_t': {'t': 5.944715282629043e-07},
          'ts.qkv_s': {'t': 5.440390764767992e-07},
          'ts.x_t': {'t': 1.4994182494420955e-06, 'r': 2.0942786924294734e-06},
          'ts.x_s': {'t': 6.744720332748581e-07, 'r': 1.3212786297162562e-06},
          'ts.mean': {'t': 8.159652672681505e-07},
          'ts.logits': {'t': 4.3207755387997586e-07},
          'ts.x_t_gated': {'t': 1.0096060965459967e-07, 'r': 1.6021997482682168e-07},
          'ts.x_s_gated': {'t': 1.2771791383798397e-07, 'r': 1.7471994210357148e-07},
          'ts.y_t': {'t': 5.428197593000083e-07},
          'ts.y_s': {'t': 7.364017137554255e-07},
          'ts.x1': {'t': 2.055791716413908e-07},
          'ts.out': {'t': 3.518430037137046e-07},
          'ts.part_o': {'t': 1.320020650053358e-06, 'r': 2.71689752762152e-06},
          'ts.part_lse': {'t': 2.1130638474300755e-07}},
 'ts:L': {'ts.qkv_t': {'t': 5.983866237465115e-07},
          'ts.qkv_s': {'t': 5.729749293409197e-07},
          'ts.x_t': {'t': 8.287369440964078e-07, 'r': 1.2322949126496986e-06},
          'ts.x_s': {'t': 6.714033952491354e-07, 'r': 1.5835284424481277e-06},
          'ts.mean': {'t': 4.5577075076626845e-06},
          'ts.logits': {'t': 3.744401534080574e-07},
          'ts.x_t_gated': {'t': 1.083072919387275e-07, 'r': 1.5811142118725294e-07},
          'ts.x_s_gated': {'t': 1.0297843907737931e-07, 'r': 1.6643366858754126e-07},
          'ts.y_t': {'t': 9.467441006022341e-07},
          'ts.y_s': {'t': 7.338617171976428e-07},
          'ts.x1': {'t': 2.3612202098199623e-07},
          'ts.out': {'t': 3.0539481646129315e-07},
          'ts.part_o': {'t': 1.5174874669102976e-06, 'r': 2.2784998324661757e-06},
          'ts.part_lse': {'t': 1.3774686300967336e-07}},
 'ts:XL': {'ts.qkv_t': {'t': 5.569077395403665e-07},
           'ts.qkv_s': {'t': 5.172184444148062e-07},
           'ts.part_o': {'t': 1.9095027344008156e-06, 'r': 2.7924794774708376e-06},
           'ts.part_lse': {'t': 1.3656120807629534e-07},
           'ts.x_t': {'t': 4.054828480978055e-07, 'r': 6.371874341880502e-07},
           'ts.x_s': {'t': 6.302064465860573e-07, 'r': 1.245573715616433e-06},
           'ts.mean': {'t': 1.2780830418076786e-05},
           'ts.logits': {'t': 2.767810137570994e-07},
           'ts.x_t_gated': {'t': 1.2283202501316655e-07, 'r': 1.768658462866588e-07},
           'ts.x_s_gated': {'t': 1.0723622143718182e-07, 'r': 1.7404116186463667e-07},
           'ts.y_t': {'t': 4.2721599789962487e-07},
           'ts.y_s': {'t': 6.79473664493506e-07},
           'ts.x1': {'t': 2.1095860311284027e-07},
           'ts.out': {'t': 3.1419600871935884e-07}},
 'ts:LN': {'ts.qkv_t': {'t': 3.966555318459553e-08},
           'ts.qkv_s': {'t': 5.038058409468123e-08},
           'ts.x_t': {'t': 1.69107570782218e-07, 'r': 1.8456203075991313e-07},
           'ts.x_s': {'t': 2.6460648618007295e-07, 'r': 3.625293958557657e-07},
           'ts.mean': {'t': 1.182492135392619e-07},
           'ts.logits': {'t': 2.2344252245707537e-07},
           'ts.x_t_gated': {'t': 9.189861722531151e-08, 'r': 9.467718542982255e-08},
           'ts.x_s_gated': {'t': 1.1423024106327832e-07, 'r': 1.3595881630030042e-07},
           'ts.y_t': {'t': 0.0},
           'ts.y_s': {'t': 0.0},
           'ts.x1': {'t': 1.0576611321982408e-07},
           'ts.out': {'t': 1.2065062299768365e-07}},
 'gru:S': {'gru.xc': {'t': 9.123323008723621e-08},
           'gru.xin': {'t': 1.222982166103438e-07},
           'gru.gi00': {'t': 6.596362922976201e-07},
           'gru.gi01': {'t': 6.670898069265056e-07},
           'gru.l0': {'t': 5.714382450253343e-07},
           'gru.gi10': {'t': 5.781371883131012e-07},
           'gru.gi11': {'t': 6.733631330003642e-07},
           'gru.l1': {'t': 2.2898588234972127e-07},
           'gru.hfin': {'t': 3.5275427524538177e-07},
           'gru.hid_speed': {'t': 4.91766005980376e-07},
           'gru.hid_step': {'t': 7.764527198360724e-07},
           'gru.hid_phase': {'t': 6.844992830385645e-07},
           'gru.avg': {'t': 1.6406681010831525e-07},
           'gru.phase': {'t': 1.9001780739080527e-07}},
 'gru:M': {'gru.xc': {'t': 8.49903340865711e-08},
           'gru.xin': {'t': 9.335524107452325e-08},
           'gru.gi00': {'t': 6.162235268822175e-07},
           'gru.gi01': {'t': 5.304881675923906e-07},
           'gru.l0': {'t': 4.579406800995727e-07},
           'gru.gi10': {'t': 6.477890016301815e-07},
           'gru.gi11': {'t': 7.243183957414301e-07},
           'gru.l1': {'t': 1.9273748484306544e-07},
           'gru.hfin': {'t': 2.2052981630790484e-07},
           'gru.hid_speed': {'t': 2.4675522866505556e-07},
           'gru.hid_step': {'t': 2.306787837217465e-07},
           'gru.hid_phase': {'t': 6.555984728675309e-07},
           'gru.avg': {'t': 1.43455618733185e-07},
           'gru.phase': {'t': 2.9213670230354746e-07}},
 'gru:L': {'gru.xc': {'t': 9.029712070116709e-08},
           'gru.xin': {'t': 1.0796374259658807e-07},
           'gru.gi00': {'t': 5.647591222853479e-07},
           'gru.gi01': {'t': 4.745986385730162e-07},
           'gru.l0': {'t': 5.151882939694811e-07},
           'gru.gi10': {'t': 6.589714523367631e-07},
           'gru.gi11': {'t': 5.947285261337858e-07},
           'gru.l1': {'t': 1.6795200180763175e-07},
           'gru.hfin': {'t': 1.6982280434817716e-07},
           'gru.hid_speed': {'t': 3.243538727042224e-07},
           'gru.hid_step': {'t': 2.992165001637573e-07},
           'gru.hid_phase': {'t': 6.73924637351845e-07},
           'gru.avg': {'t': 2.1703485759921442e-07},
           'gru.phase': {'t': 3.8644767483895384e-07}},
 'fc:S': {'fc.cparams': {'t': 1.3560879588141394e-07},
          'fc.hid_t': {'t': 1.3215202843355138e-07},
          'fc.g_s': {'t': 3.306275019137909e-07},
          'fc.g_t': {'t': 6.702737065287061e-07},
          'fc.y': {'t': 1.3862883165050477e-07},
          'fc.y_s': {'t': 1.0721467903048367e-07},
          'fc.out': {'t': 5.4263580403825764e-08}},
 'fc:L': {'fc.cparams': {'t': 1.2625730512225005e-07},
          'fc.hid_t': {'t': 1.659779579583727e-07},
          'fc.g_s': {'t': 3.8983694056837866e-07},
          'fc.g_t': {'t': 7.082193958186126e-07},
          'fc.y': {'t': 1.4594837052462608e-07},
          'fc.y_s': {'t': 1.4282941940948897e-07},
          'fc.out': {'t': 4.6548686615424395e-08}}}
# END FLOORS


def floor(stage, cls, metric="t"):
    module = stage.split(".")[0]
    return FLOORS[f"{module}:{cls}"][stage][metric]


def bar(stage, cls, metric="t"):
    return min(FLOOR_FACTOR * floor(stage, cls, metric), MODULE_BAR[stage.split(".")[0]])


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def row_err(a, b, heads=1):
    """Worst last-axis vector (split into `heads` equal parts): max |a - b| over the vector / max |b| over it."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a = a.reshape(-1, heads, a.shape[-1] // heads)
    b = b.reshape(a.shape)
    return float((np.abs(a - b).max(-1) / np.maximum(np.abs(b).max(-1), 1e-30)).max())


def stage_errors(stage, got, ref):
    """{metric: error} of one stage's output against its reference."""
    assert got.shape == ref.shape, (stage, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{stage}: non-finite values"
    e = {"t": rel_err(got, ref)}
    if stage in ROW_STAGES:
        e["r"] = row_err(got, ref, heads=4)
    return e


def check_stage(stage, cls, got, ref, log=None, label=""):
    """Assert every metric of the stage under its bar; returns {metric: (error, bar)}.  `log`: a list that receives one text line per metric."""
    out, bad = {}, []
    for metric, err in stage_errors(stage, got, ref).items():
        lim = bar(stage, cls, metric)
        out[metric] = (err, lim)
        if log is not None:
            log.append(f"{label:14s} {stage:16s} {metric} class {cls:2s} floor {floor(stage, cls, metric):.2e} bar {lim:.2e} error {err:.2e}")
        if not err <= lim:
            bad.append(f"{stage} [{metric}] {label}: error {err:.3e} above the bar {lim:.3e} (fp32 floor {floor(stage, cls, metric):.2e})")
    assert not bad, "; ".join(bad)
    return out


def report(lines):
    """Print figures (before anything is asserted on them); GRNET_STAGE_ERRORS_LOG=<file> also appends them there (profiles/temporal_stage_errors.md)."""
    import os
    for line in lines:
        print(line)
    path = os.environ.get("GRNET_STAGE_ERRORS_LOG")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------------------------------------- where a walker's inputs come from
class HostSource:
    """The fp32 restatement feeds itself: every stage's float32 output is kept and read by the stages behind it."""
    restate = True

    def __init__(self, **inputs):
        self.t = {k: np.asarray(v, np.float32) for k, v in inputs.items()}

    def get(self, name, rows=None):
        a = self.t[name]
        return a if rows is None else a[:, rows]

    def put(self, name, value):
        self.t[name] = np.asarray(value, np.float32)


class TapSource:
    """The taps of one GPU call (torch tensors on the device, shaped (b, n, ...)) plus the call's inputs; rows are selected on the device."""
    restate = False

    def __init__(self, tensors):
        self.t = tensors

    def get(self, name, rows=None):
        a = self.t[name]
        if rows is not None:
            import torch
            a = a.index_select(1, torch.as_tensor(np.asarray(rows), device=a.device))
        return a.cpu().numpy()


def flash_key_parts(n, cus, max_parts=8, min_part_keys=128, tile=128, heads=4):
    """The launcher's rule for the blocked kernel (tsattn_kernels.hip: flash_key_parts) restated: the key-part count that minimises rounds of workgroups
    per part on `cus` CUs, no part shorter than 128 keys, clips of more than 8 192 frames in parts of at most 4 096 keys."""
    wgs = (n + tile - 1) // tile * heads
    pmin = 1 if n <= 8192 else min(max_parts, (n + 4095) // 4096)      # beyond 8 192 frames a part is at most 4 096 keys (rounding of the sequential accumulators)
    best, best_cost = pmin, 1e30
    for p in range(pmin, max_parts + 1):
        if p > 1 and n // p < min_part_keys:
            break
        cost = ((wgs * p + cus - 1) // cus) / p + 0.01 * p
        if cost < best_cost - 1e-9:
            best_cost, best = cost, p
    return best


def sample_rows(n, count=1024, seed=20240607):
    """The query rows checked of a clip too long to check whole: the first and last 16, both sides of every 128-row query-tile seam among a random 32 tiles,
    random rows for the rest (fixed seed); sorted, unique, exactly `count`."""
    g = np.random.Generator(np.random.Philox(key=[seed, n]))
    rows = set(range(16)) | set(range(n - 16, n))
    tiles = g.choice(np.arange(1, (n + 127) // 128), size=32, replace=False)
    for t in tiles:
        rows |= {int(t) * 128 - 1, int(t) * 128}
    pool = g.permutation(n)
    for r in pool:
        if len(rows) >= count:
            break
        rows.add(int(r))
    return np.array(sorted(rows))


# ------------------------------------------------------------------------------------------------- the walkers
def _both(oracle, src, fn):
    """(got, reference) of one stage: reference = fn() under float64(); got = fn() in plain float32 when the source restates, else None."""
    with oracle.float64():
        ref = fn()
    return (fn() if src.restate else None), ref


def ts_walk(oracle, sd, src, b, n, parts, rows=None, prefix="ts.", x_name="x", xs_name="xs"):
    """The attention block launch by launch.  src holds x (b,n,3072), xs (b,n,3200) and -- a TapSource -- every tap shaped (b,n,...) / (parts,b,n,...).
    rows: the frames of each clip that are checked (None: all); the clip mean always takes every frame.  Yields (stage, got, ref)."""
    P = lambda k: sd["mulattn." + k]
    R = lambda a: a.reshape(-1, a.shape[-1])
    nr = n if rows is None else len(rows)

    def stage(name, fn, shape=None):
        got, ref = _both(oracle, src, fn)
        if src.restate:
            src.put(prefix + name, got)
        else:
            got = src.get(prefix + name, rows if shape is None else None)
        return prefix + name, got.reshape(ref.shape), ref

    def full(name):
        """Every frame of a tensor the restatement computed on the sampled rows only: the sampled rows repeated cyclically (same distribution, n rows)."""
        a = src.get(prefix + name)
        return a if a.shape[1] == n else a[:, np.resize(np.arange(a.shape[1]), n)]

    x, xs = src.get(x_name, rows), src.get(xs_name, rows)
    yield stage("qkv_t", lambda: oracle.linear(x, P("qkv_t.weight"), P("qkv_t.bias")))
    yield stage("qkv_s", lambda: oracle.linear(xs, P("qkv_s.weight"), P("qkv_s.bias")))
    if src.restate and rows is not None:                       # the keys and values of every frame (fp32 GEMM on all rows; only the sampled rows are compared above)
        qkv_full = np.asarray(oracle.linear(src.get(x_name), P("qkv_t.weight"), P("qkv_t.bias")), np.float32)
    else:
        qkv_full = src.get(prefix + "qkv_t")
    if parts > 1:
        o_ref, l_ref, o_got, l_got = [], [], [], []
        for p, kr in enumerate(oracle.ts_key_part_ranges(n, parts)):
            with oracle.float64():
                o, l = oracle.ts_stage_temporal_attention(qkv_full, rows, key_range=kr, partial=True)
            o_ref.append(o), l_ref.append(l)
            if src.restate:
                o, l = oracle.ts_stage_temporal_attention(qkv_full, rows, key_range=kr, partial=True)
                o_got.append(o), l_got.append(l)
        if not src.restate:                                    # (O, m, l) as the kernel left them -> O / l and m + log2 l in float64
            t_o, t_ml = src.t[prefix + "part_o"], src.t[prefix + "part_ml"]
            for p in range(parts):
                sub = TapSource({"o": t_o[p], "ml": t_ml[p]})
                o, ml = sub.get("o", rows).astype(np.float64), sub.get("ml", rows).astype(np.float64)
                l = ml[..., 1]
                o_got.append(o / np.repeat(l, o.shape[-1] // l.shape[-1], -1))
                l_got.append(ml[..., 0] + np.log2(l))
        yield prefix + "part_o", np.stack(o_got), np.stack(o_ref)
        yield prefix + "part_lse", np.stack(l_got), np.stack(l_ref)
    yield stage("x_t", lambda: oracle.ts_stage_temporal_attention(qkv_full, rows))
    qs = src.get(prefix + "qkv_s", rows) if not src.restate else src.get(prefix + "qkv_s")
    yield stage("x_s", lambda: oracle.ts_stage_spatial_attention(R(qs)).reshape(b, nr, -1))
    xt_all, xs_all = (full("x_t"), full("x_s")) if src.restate else (src.get(prefix + "x_t"), src.get(prefix + "x_s"))
    yield stage("mean", lambda: oracle.ts_stage_clip_mean(xt_all, xs_all), shape="clip")
    mean = src.get(prefix + "mean")
    yield stage("logits", lambda: oracle.linear(mean, P("ts_attn.weight"), P("ts_attn.bias")), shape="clip")
    logits = src.get(prefix + "logits")
    xt_r, xs_r = (src.get(prefix + "x_t"), src.get(prefix + "x_s")) if src.restate else (src.get(prefix + "x_t", rows), src.get(prefix + "x_s", rows))
    got, ref = _both(oracle, src, lambda: oracle.ts_stage_gate_apply(logits, xt_r, xs_r))
    for i, name in enumerate(("x_t_gated", "x_s_gated")):
        if src.restate:
            src.put(prefix + name, got[i])
        yield prefix + name, (got[i] if src.restate else src.get(prefix + name, rows)), ref[i]
    g = lambda name: src.get(prefix + name) if src.restate else src.get(prefix + name, rows)
    xtg, xsg = g("x_t_gated"), g("x_s_gated")
    yield stage("y_t", lambda: oracle.linear(xtg, P("fc_t.weight"), P("fc_t.bias")))
    yield stage("y_s", lambda: oracle.linear(xsg, P("fc_s.weight"), P("fc_s.bias")))
    yt, ys = g("y_t"), g("y_s")
    yield stage("x1", lambda: oracle.ts_stage_residual_ln(x, yt, ys, sd))
    x1 = g("x1")
    yield stage("out", lambda: oracle.ts_stage_jwff_ln(x1, sd))


def gru_walk(oracle, sd, src, b, T, prefix="gru.", x_name="x", cp_name="cparams"):
    """The GRU encoder launch by launch.  src holds x (b,T,3072), cparams (b,T,3) and -- a TapSource -- every tap shaped (b,T,...) / (b,...)."""
    def stage(name, fn, pick=None):
        got, ref = _both(oracle, src, fn)
        if pick is not None:
            got, ref = (None if got is None else got[pick]), ref[pick]
        if src.restate:
            src.put(prefix + name, got)
        else:
            got = src.get(prefix + name)
        return prefix + name, got.reshape(ref.shape), ref

    x, cp = src.get(x_name), src.get(cp_name)
    yield stage("xc", lambda: oracle.gru_stage_prep(x, cp, sd), pick=0)
    yield stage("xin", lambda: oracle.gru_stage_prep(x, cp, sd), pick=1)
    layer_in = src.get(prefix + "xin")
    fin_got, fin_ref = [], []
    for layer in range(2):
        for d, suf in enumerate(("", "_reverse")):
            yield stage(f"gi{layer}{d}", lambda: oracle.linear(layer_in, sd[f"rnn.weight_ih_l{layer}{suf}"], sd[f"rnn.bias_ih_l{layer}{suf}"]))
        got, ref = [], []
        for d, suf in enumerate(("", "_reverse")):             # each direction's recurrence on its own tapped gi
            gi = src.get(prefix + f"gi{layer}{d}")
            g, r = _both(oracle, src, lambda: oracle.gru_stage_recurrence(gi, sd[f"rnn.weight_hh_l{layer}{suf}"], sd[f"rnn.bias_hh_l{layer}{suf}"], bool(d)))
            ref.append(r[0]), fin_ref.append(r[1])
            if src.restate:
                got.append(g[0]), fin_got.append(g[1])
        ref = np.concatenate(ref, -1)
        if src.restate:
            src.put(prefix + f"l{layer}", np.concatenate(got, -1))
        yield prefix + f"l{layer}", src.get(prefix + f"l{layer}").reshape(ref.shape), ref
        layer_in = src.get(prefix + f"l{layer}")
    ref = np.concatenate(fin_ref, -1)
    if src.restate:
        src.put(prefix + "hfin", np.concatenate(fin_got, -1))
    yield prefix + "hfin", src.get(prefix + "hfin").reshape(ref.shape), ref
    hf = src.get(prefix + "hfin")
    yield stage("hid_speed", lambda: oracle.linear(hf, sd["speed_mlp.0.weight"], sd["speed_mlp.0.bias"]))
    yield stage("hid_step", lambda: oracle.linear(hf, sd["step_mlp.0.weight"], sd["step_mlp.0.bias"]))
    yield stage("hid_phase", lambda: oracle.linear(layer_in, sd["phase_mlp.0.weight"], sd["phase_mlp.0.bias"]))
    hs, ht, hp = src.get(prefix + "hid_speed"), src.get(prefix + "hid_step"), src.get(prefix + "hid_phase")
    yield stage("avg", lambda: np.concatenate([oracle.gru_stage_mlp_out(hs, sd, "speed_mlp"), oracle.gru_stage_mlp_out(ht, sd, "step_mlp")], -1))
    yield stage("phase", lambda: oracle.gru_stage_mlp_out(hp, sd, "phase_mlp", act_tanh=True))


def fc_walk(oracle, sd, src, b, n, parts, ts_rows=None, p="pfeat_corrector."):
    """grnet_gait_correct's temporal launches in order: src holds cam (b,n,3), bbox (b,n,4), cimg (b,n,2), x (b,n,3072) -- cparams, the GRU on (x, cparams)
    (gru_walk), hid_t, g_s, g_t, y, y_s, the attention block on (y, y_s) (ts_walk, on the frames ts_rows of each clip), out."""
    def stage(name, fn, pick=None):
        got, ref = _both(oracle, src, fn)
        if pick is not None:
            got, ref = (None if got is None else got[pick]), ref[pick]
        if src.restate:
            src.put("fc." + name, np.asarray(got).reshape(b, n, -1))
        else:
            got = src.get("fc." + name)
        return "fc." + name, np.asarray(got).reshape(ref.shape), ref

    tsd = {k[len(p + "featTencoder.0."):]: v for k, v in sd.items() if k.startswith(p + "featTencoder.0.")}
    cam, bbox, cimg, x = src.get("cam"), src.get("bbox"), src.get("cimg"), src.get("x")
    yield stage("cparams", lambda: oracle.gait_cparams(cam.reshape(-1, 3), bbox, cimg))
    gsd = {k[len(p + "featnet."):]: v for k, v in sd.items() if k.startswith(p + "featnet.")}
    yield from gru_walk(oracle, gsd, src, b, n, x_name="x", cp_name="fc.cparams")
    avg, phase = src.get("gru.avg"), src.get("gru.phase")
    yield stage("hid_t", lambda: oracle.fc_stage_hidden(avg, phase, sd, p), pick=0)
    yield stage("g_s", lambda: oracle.fc_stage_hidden(avg, phase, sd, p), pick=1)
    hid_t, g_s = src.get("fc.hid_t"), src.get("fc.g_s")
    yield stage("g_t", lambda: oracle.linear(hid_t, sd[p + "gfeat_mpl_t.3.weight"], sd[p + "gfeat_mpl_t.3.bias"]))
    g_t = src.get("fc.g_t")
    flat = lambda a: a.reshape(b * n, -1)
    yield stage("y", lambda: oracle.fc_stage_bn(flat(x), flat(g_t), flat(g_s), sd, p), pick=0)
    yield stage("y_s", lambda: oracle.fc_stage_bn(flat(x), flat(g_t), flat(g_s), sd, p), pick=1)
    yield from ts_walk(oracle, tsd, src, b, n, parts, rows=ts_rows, x_name="fc.y", xs_name="fc.y_s")
    if src.restate:
        src.put("fc.att", src.get("ts.out"))
    att = src.get("fc.att", None if src.restate else ts_rows)   # the rows the attention block was checked on (a restating source holds only those)
    xr = src.get("x", ts_rows)
    dt = lambda: np.float64 if oracle._F64 else np.float32
    got, ref = _both(oracle, src, lambda: np.asarray(att, dt()) + np.asarray(xr, dt()))
    yield "fc.out", (got if src.restate else src.get("fc.out", ts_rows)).reshape(ref.shape), ref


def make_gait_inputs(pkg, b, n):
    """cam (b,n,3) [s, tx, ty] and boxes that are neither 224 wide nor centred (synth.make_gait_boxes: 180 .. 420 wide, anywhere in a 1920 x 1080 image)."""
    _, cam = pkg.synth.make_featcorr_inputs(b, n)
    bbox, cimg = pkg.synth.make_gait_boxes(b, n)
    return cam, bbox, cimg


def low_variance_case(pkg, b=1, n=16):
    """An attention block whose two LayerNorms see rows of standard deviation 1e-3, where (std + eps) and sqrt(var + eps) differ by 40 % (on rows of unit
    variance they differ by 5e-7, under fp32 resolution): fc_t, fc_s and the JWFF weights are zero, so LN1 normalises x itself and LN2 normalises x1, and
    x = 1e-3 x noise, norm1.gamma = 1e-3.  -> (state dict, x (b,n,128,24), xs (b,n,128,25)); size class "LN"."""
    sd = dict(pkg.synth.make_tsattn_state_dict())
    for k in ("mulattn.fc_t.weight", "mulattn.fc_t.bias", "mulattn.fc_s.weight", "mulattn.fc_s.bias", "ffn.jwff_layer1.weight", "ffn.jwff_layer2.weight"):
        sd[k] = np.zeros_like(sd[k])
    sd["norm1.gamma"] = np.full_like(sd["norm1.gamma"], 1e-3)
    sd["norm1.beta"] = np.zeros_like(sd["norm1.beta"])
    x, xs = pkg.synth.make_tsattn_inputs(b, n)
    return sd, (x * np.float32(1e-3)).astype(np.float32), (xs * np.float32(1e-3)).astype(np.float32)
