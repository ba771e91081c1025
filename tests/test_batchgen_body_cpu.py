"""batch_generation.py --gait_body through the model_factory / gloo seam of the CPU tests, on one rank and on two: a stand-in whose
vertices are a real torus over synth.make_faces() (radii 0.6 and 0.2, scaled and moved by a function of the frame's pixels, turned inside out where
its eighth pixel is above 1 (the one-frame video among them)), the JSON file keyed by pipeline.BODY_COLUMNS with null where a value is undefined, the two database columns and nothing
else new, one 'Body:' line per video, the eleven doubles through the window's one all-gather as 22 float32 words without the loss of a bit (NaN
payloads included), the device method called once per work item on the tensor the forward returned, --balance_com mesh handing WindowBalance the very
centres, and every refusal of the new flags."""
import importlib
import json
import multiprocessing as mp
import os
import socket
import sys

import numpy as np
import pytest

from .conftest import PKG_NAME, ROOT
from .helpers import body_checks as bc
from .test_host_cpu import _StandInModel, _write_video_dir

LENGTHS = [7, 23, 3, 12, 1]
CHUNK = 8
PAYLOAD = np.array([0x7FF8000000ABCDEF], np.uint64).view(np.float64)[0]      # a quiet NaN that carries a number


@pytest.fixture(scope="module")
def bg():
    sys.path.insert(0, ROOT)
    return importlib.import_module("batch_generation")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import joblib
    root = str(tmp_path_factory.mktemp("batchgen_body"))
    fv, vid_folder = _write_video_dir(root, LENGTHS)
    return {"root": root, "fv": fv, "vid_folder": vid_folder, "annos": joblib.load(fv)}


class _BodyStandIn(_StandInModel):
    """The stand-in's joints, and a mesh: the torus over synth.make_faces(), its size and place a fixed function of the frame's pixels."""
    forwards = []

    def __init__(self):
        synth = importlib.import_module(PKG_NAME).synth
        self.faces = synth.make_faces()
        self.torus = bc.torus_points(65, 106).astype(np.float32)

    def __call__(self, x):
        import torch
        out = super().__call__(x)[0]
        f = x[0].reshape(x.shape[1], -1)
        scale = 1.0 + 0.05 * torch.tanh(f[:, 1])
        shift = torch.stack([f[:, 2], f[:, 3], 3.0 + 0.1 * f[:, 4]], 1)
        verts = torch.from_numpy(self.torus)[None] * scale[:, None, None]
        verts = torch.where((f[:, 7] > 1.0)[:, None, None], verts * torch.tensor([1.0, 1.0, -1.0]), verts) + shift[:, None, :]
        out["verts"] = verts.to(torch.float32).unsqueeze(0).contiguous()
        type(self).forwards.append(out["verts"])
        return [out]


class _BodyStandInWithMethod(_BodyStandIn):
    """... with the device method's signature, answered by the host statement; a row whose volume's sixth decimal is a multiple of 5 gets a NaN with a
    payload in its last moment, so that the gather is seen to carry payloads."""
    calls = []

    def mesh_moments(self, verts, return_sums=False):
        import torch
        pipe = importlib.import_module(PKG_NAME).pipeline
        type(self).calls.append(verts)
        rows = pipe.mesh_moments(verts.numpy(), self.faces)
        rows[np.floor(np.abs(rows[:, 0]) * 1e6) % 5 == 0, 9] = PAYLOAD
        return torch.from_numpy(rows)

    def gait_parameters(self, joints3d, lengths=None, trans=None, **kw):
        import torch
        pipe = importlib.import_module(PKG_NAME).pipeline
        out = pipe.gait_parameters(joints3d.cpu().numpy(), lengths=lengths, trans=trans, **kw)
        return {k: torch.from_numpy(np.asarray(v)) for k, v in out.items()}

    balance_calls = []

    def gait_balance(self, joints3d, events, lengths=None, com=None, **kw):
        import torch
        pipe = importlib.import_module(PKG_NAME).pipeline
        type(self).balance_calls.append(com)
        out = pipe.gait_balance(joints3d.cpu().numpy(), events.cpu().numpy(), lengths, com=None if com is None else com.numpy(), **kw)
        return {k: torch.from_numpy(v) for k, v in out.items() if k != "rel"}


def generate(bg, world, name, factory=lambda r: _BodyStandIn(), **kw):
    import joblib
    written = bg.prepare_data(None, world["vid_folder"], os.path.join(world["root"], name), max_frames=CHUNK, chunk=CHUNK, model_factory=factory, backend="gloo",
                              annos={k: v.copy() for k, v in world["annos"].items()}, **kw)
    assert len(written) == 1
    return joblib.load(written[0])


def test_body_on_host_writes_the_json_and_the_columns(bg, pkg, world, capsys):
    pipe = pkg.pipeline
    plain = generate(bg, world, "plain.json")
    assert "body_com" not in plain and not os.path.exists(os.path.join(world["root"], "plain_body.json"))
    capsys.readouterr()
    db = generate(bg, world, "shape.json", body={"density": 1000.0})
    printed = capsys.readouterr().out
    N = sum(LENGTHS)
    assert list(db) == list(plain) + ["body_com", "body_volume"] and all(np.array_equal(db[k], plain[k]) for k in plain)      # the two columns and nothing else
    assert db["body_com"].dtype == np.float32 and db["body_com"].shape == (N, 3) and db["body_volume"].dtype == np.float32 and db["body_volume"].shape == (N,)
    flipped = db["body_volume"] < 0
    print(f"{int(flipped.sum())} of {N} frames are inside out; volumes {db['body_volume'][:5].tolist()}")
    assert 0 < flipped.sum() < N and np.isnan(db["body_com"][flipped]).all() and np.isfinite(db["body_com"][~flipped]).all()
    assert np.allclose(np.abs(db["body_volume"]), 0.4727, rtol=0.2)                     # the torus, scaled by up to 1.05 a side
    path = os.path.join(world["root"], "shape_body.json")
    text = open(path).read()
    found = json.loads(text)
    names = np.asarray(db["vid_name"])
    keys = sorted(set(names))
    assert sorted(found) == keys and len(keys) == len(LENGTHS) and "NaN" not in text
    empty = 0
    for key in keys:
        assert list(found[key]) == list(pipe.BODY_COLUMNS) + ["density"] and found[key]["density"] == 1000.0
        sel = names == key
        assert found[key]["frames"] == sel.sum() and found[key]["frames_valid"] == (~flipped[sel]).sum()
        if found[key]["frames_valid"] == 0:
            empty += 1
            assert all(found[key][c] is None for c in pipe.BODY_COLUMNS[2:])
        else:
            assert abs(found[key]["volume_mean"] - db["body_volume"][sel][~flipped[sel]].astype(np.float64).mean()) < 1e-6
            assert found[key]["mass"] == 1000.0 * found[key]["volume_mean"] and found[key]["com_distance_mean"] > 0
    assert empty >= 1 and "null" in text                           # the one-frame video is inside out: every mean of it is null
    lines = [ln for ln in printed.splitlines() if ln.startswith("Body:")]
    assert len(lines) == len(LENGTHS) and all(all(w in ln for w in ("frames with a volume, volume", "CV", "mass", "at 1000 kg/m^3", "centre of mass")) for ln in lines)
    assert lines[0].startswith("Body: video S001C001P001R001A001, ") and all(ln.endswith(".") for ln in lines)
    assert f"Save body measures of {len(LENGTHS)} videos to {path}." in printed
    # the rows behind the file are the statement's on the stand-in's own vertices
    model = _BodyStandIn()
    crop = np.load(os.path.join(world["vid_folder"], "S003C001P001R001A003", "000001.npy"))
    import torch
    verts = model(torch.from_numpy(crop)[None, None])[0]["verts"][0]
    row = pipe.mesh_moments(verts.numpy(), model.faces)[0]
    at = np.flatnonzero(names == "S003C001P001R001A003")[1]
    assert np.array_equal(db["body_volume"][at], np.float32(row[0])) and np.array_equal(db["body_com"][at], row[1:4].astype(np.float32), equal_nan=True)


def test_device_method_once_per_work_item_and_the_very_com(bg, pkg, world, monkeypatch):
    S = _BodyStandInWithMethod
    S.calls.clear(), S.forwards.clear(), S.balance_calls.clear()
    shapes = []
    real = bg.WindowBody.add_window

    def recording(self, keys, per_video, rows):
        shapes.append(self)
        return real(self, keys, per_video, rows)
    monkeypatch.setattr(bg.WindowBody, "add_window", recording)
    db = generate(bg, world, "method.json", factory=lambda r: S(), body={}, gait={"window": 3, "sigma": 1.0}, balance={"com": "mesh", "window": 1, "settle": 0})
    items = pkg.harness.plan_work_items(LENGTHS, 1, CHUNK)
    assert len(S.calls) == len(S.forwards) == len(items) >= len(LENGTHS)                # once per work item: a forward, then the moments of its vertices
    for verts, made in zip(S.calls, S.forwards):
        assert verts.data_ptr() == made.data_ptr() and tuple(verts.shape) == tuple(made.shape[1:])      # the tensor the forward returned, where it lies
    assert len(shapes) == 1 and len(S.balance_calls) == 1 and S.balance_calls[0] is shapes[0].com       # the very centres, not a copy
    assert tuple(shapes[0].com.shape) == (sum(LENGTHS), 3) and "footprints_phase" in db and "body_com" in db
    assert os.path.isfile(os.path.join(world["root"], "method_body.json")) and os.path.isfile(os.path.join(world["root"], "method_balance.json"))
    # without --balance_com the balance call gets no centre, as before
    S.balance_calls.clear()
    generate(bg, world, "table.json", factory=lambda r: S(), body={}, gait={"window": 3, "sigma": 1.0}, balance={"window": 1, "settle": 0})
    assert S.balance_calls == [None]
    with pytest.raises(ValueError, match="needs body"):
        generate(bg, world, "nobody.json", gait={}, balance={"com": "mesh"})
    with pytest.raises(ValueError, match="'table' or 'mesh'"):
        generate(bg, world, "what.json", gait={}, balance={"com": "joints"}, body={})


def test_the_float32_view_loses_nothing(pkg):
    """Doubles -- subnormals, infinities, NaNs with payloads of either sign -- as 22 float32 words beside 75 floats through gather_work_items and back."""
    import torch
    rows = np.random.default_rng(2).standard_normal((5, 11))
    words = rows.view(np.uint64)
    words[0, :4] = [0x7FF8000000ABCDEF, 0xFFF8000000000001, 0x7FF0000000000000, 0x0000000000000001]
    words[3, 10] = 0x7FF4000000000000 | 0x0008000000000000          # quiet, with a payload in the low float32 word's neighbour
    body = torch.from_numpy(rows.copy())
    joints = torch.arange(5 * 75, dtype=torch.float32).reshape(5, 75)
    local = torch.cat([joints, body.contiguous().view(torch.float32).reshape(5, 22)], 1)
    assert local.shape == (5, 97) and local.dtype == torch.float32
    got = pkg.harness.gather_work_items([(0, 0, 2, 0), (1, 0, 3, 0)], local, 97, 1, 0, None, torch.device("cpu"))
    back = torch.cat([got[0], got[1]])[:, 75:].clone(memory_format=torch.contiguous_format).view(torch.float64).numpy()
    assert np.array_equal(back.view(np.uint64), rows.view(np.uint64))


def _body_worker(rank, world_size, port, root, fv, vid_folder, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world_size), RANK=str(rank), LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
    bg = importlib.import_module("batch_generation")
    real = bg.WindowBody.add_window

    def recording(self, keys, per_video, rows):
        import torch
        np.save(os.path.join(root, f"rows_w{world_size}.npy"), torch.cat([rows[vi] for vi in range(len(keys))], 0).numpy().view(np.uint64))
        return real(self, keys, per_video, rows)
    bg.WindowBody.add_window = recording
    written = bg.prepare_data(fv, vid_folder, os.path.join(root, f"both_w{world_size}.json"), max_frames=CHUNK, chunk=CHUNK,
                              model_factory=lambda r: _BodyStandInWithMethod(), backend="gloo", body={})
    q.put((rank, written))


def test_two_gloo_ranks_equal_one_process(world):
    """The rows rank 0 holds after the two-rank gather against the one-rank rows: every bit, the payloads the stand-in plants included; the database
    and the JSON file alike."""
    import joblib
    dbs, rows = {}, {}
    for size in (1, 2):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        procs = [ctx.Process(target=_body_worker, args=(r, size, port, world["root"], world["fv"], world["vid_folder"], q)) for r in range(size)]
        for p in procs:
            p.start()
        res = dict(q.get(timeout=180) for _ in procs)
        for p in procs:
            p.join(timeout=60)
        assert len(res[0]) == 1 and all(res[r] == [] for r in range(1, size)), res
        dbs[size], rows[size] = joblib.load(res[0][0]), np.load(os.path.join(world["root"], f"rows_w{size}.npy"))
    assert rows[1].shape == (sum(LENGTHS), 11) and np.array_equal(rows[1], rows[2])
    planted = rows[1][:, 9] == np.array([PAYLOAD]).view(np.uint64)[0]
    print(f"{int(planted.sum())} rows carry the planted payload")
    assert planted.any() and not planted.all()
    assert list(dbs[1]) == list(dbs[2]) and all(np.array_equal(dbs[1][k], dbs[2][k], equal_nan=dbs[1][k].dtype.kind == "f") for k in dbs[1])
    assert open(os.path.join(world["root"], "both_w1_body.json")).read() == open(os.path.join(world["root"], "both_w2_body.json")).read()


def test_main_runs_body_on_host(bg, world, tmp_path, monkeypatch):
    """The flags reach prepare_data: main with the seam's arguments patched in."""
    import joblib
    seen = {}
    real = bg.prepare_data

    def patched(**kw):
        seen.update(body=kw["body"], balance=kw["balance"])
        return real(**{**kw, "fv": None, "annos": {k: v.copy() for k, v in world["annos"].items()}, "model_factory": lambda r: _BodyStandIn(), "backend": "gloo",
                       "max_frames": CHUNK, "chunk": CHUNK})
    monkeypatch.setattr(bg, "prepare_data", patched)
    outpath = str(tmp_path / "main.json")
    bg.main(["--bbox_path", world["fv"], "--vid_folder", world["vid_folder"], "--outpath", outpath, "--gait", "--gait_on_host", "--gait_balance", "--balance_on_host",
             "--gait_body", "--body_on_host", "--body_density", "1010", "--balance_com", "mesh"])
    assert seen["body"] == {"density": 1010.0, "on_host": True, "out": None} and seen["balance"]["com"] == "mesh"
    assert sorted(json.load(open(str(tmp_path / "main_body.json")))) == sorted(world["annos"]) and os.path.isfile(str(tmp_path / "main_balance.json"))
    db = joblib.load(str(tmp_path / "main_0.json"))
    assert "body_com" in db and "body_volume" in db and "footprints_phase" in db


def test_body_flags_are_refused_where_they_do_not_belong(bg):
    base = ["--bbox_path", "a.pkl", "--vid_folder", "v"]
    for argv, word in ((["--body_out", "b.json"] + base, "--body_out belongs to --gait_body"), (["--body_density", "985"] + base, "--body_density belongs to --gait_body"),
                       (["--body_on_host"] + base, "--body_on_host belongs to --gait_body"),
                       (["--gait_body", "--bbox_path", "a.pkl"], "--gait_body needs --vid_folder"),
                       (["--gait_body", "--body_density", "0"] + base, "--body_density must be"), (["--gait_body", "--body_density", "nan"] + base, "--body_density must be"),
                       (["--gait_body", "--body_density", "-1"] + base, "--body_density must be"),
                       (["--gait_body", "--balance_com", "mesh"] + base, "--balance_com belongs to --gait_balance"),
                       (["--gait", "--balance_com", "table"] + base, "--balance_com belongs to --gait_balance"),
                       (["--gait", "--gait_balance", "--balance_com", "mesh"] + base, "--balance_com mesh needs --gait_body")):
        with pytest.raises(SystemExit) as e:
            bg.main(argv)
        assert isinstance(e.value.code, str) and word in e.value.code and len(e.value.code.splitlines()) == 1, argv
    with pytest.raises(SystemExit) as e:                           # argparse's own refusal of another choice
        bg.main(["--gait", "--gait_balance", "--gait_body", "--balance_com", "joints"] + base)
    assert e.value.code == 2
