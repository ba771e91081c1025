"""Time of the 3D skeleton view (GRNet.render_segments = grnet_render_segments), by HIP events, on one MI355X:

    chunk_ms   what demo.py --skeleton_view asks of the device per chunk of 16 frames of 1920 x 1080: the white panel, one call for the grid of
               all 16 panels, one call for the skeletons of all their persons (P = 1, 4 per frame; the 27 SPIN bones of seeded joints, width 13).
               The panels are resident on the device; the tables of a call come from host memory, as in the demo.  Median of REPS runs after a
               warm one.
    matplotlib_s_per_frame   where matplotlib can be imported: the reference's figure (input panel + 3D axes with the same bones) through savefig to
               memory, on THIS machine's CPU, median of 5 frames after a warm one; "-" otherwise.

Records, not bars: nothing existed before to compare against.  The whole run is under a time limit of LIMIT_S seconds (SIGALRM).

    python tools/skeleton_time.py [path]        writes the file whole; default: profiles/skeleton_times.txt
"""
import importlib
import io
import os
import signal
import statistics
import sys
import time

REPS = 10
FRAMES = 16
H, W = 1080, 1920
LIMIT_S = 300


def matplotlib_seconds(pipe, joints, np):
    try:
        import matplotlib
    except ImportError:
        return None
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    bones, colours = pipe.skeleton_bones("spin")
    fig = plt.figure("Video")
    ax_in = fig.add_subplot(1, 2, 1)
    ax = fig.add_subplot(1, 2, 2, projection="3d")
    frame = np.zeros((H, W, 3), np.uint8)
    ts = []
    for k in range(6):
        t0 = time.perf_counter()
        ax_in.clear()
        ax_in.set_axis_off()
        ax_in.imshow(frame, aspect="equal")
        ax.clear()
        ax.view_init(elev=pipe.SKELETON_ELEV, azim=pipe.SKELETON_AZIM)
        for lim, setter, ticks in zip(pipe.SKELETON_LIMITS, (ax.set_xlim3d, ax.set_ylim3d, ax.set_zlim3d), pipe.SKELETON_TICKS):
            setter(list(lim))
        for (a, b), c in zip(bones, colours):
            ax.plot(*[joints[[a, b], d] for d in range(3)], lw=2, c=tuple(c / 255.0))
        fig.savefig(io.BytesIO(), format="png")
        ts.append(time.perf_counter() - t0)
    plt.close(fig)
    return statistics.median(ts[1:])


def main():
    signal.alarm(LIMIT_S)
    import numpy as np
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    pipe = pkg.pipeline
    assert torch.cuda.is_available(), "skeleton_time.py measures on the GPU"
    m = pkg.build_synthetic_model(max_frames=2, with_gru=False, compact_arena=True)
    bones, colours = pipe.skeleton_bones("spin")
    grid_points, grid_segments = pipe.skeleton_grid()
    S = min(H, W)
    bone_w, grid_w = max(2, round(S / 81)), max(1, round(S / 203))
    panel = torch.empty(FRAMES, H, W, 3, dtype=torch.uint8, device="cuda")
    grid = np.repeat(grid_points[None], FRAMES, 0)
    R = np.eye(3)

    def events(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    lines = [f"# the 3D skeleton view on one MI355X: a chunk of {FRAMES} panels of {W} x {H}, resident on the device: white, the grid ({len(grid_segments)} segments, width {grid_w}),",
             f"# then P persons per frame ({len(bones)} bones, width {bone_w}); chunk_ms: median of {REPS} HIP-event times after a warm run (tools/skeleton_time.py)",
             "# persons chunk_ms ms_per_frame non_white_pixels_per_frame matplotlib_s_per_frame"]
    g = np.random.Generator(np.random.Philox(key=[0, 7]))
    for persons in (1, 4):
        joints = (g.standard_normal((FRAMES * persons, 49, 3)) * (0.2, 0.3, 0.3)).astype(np.float32)
        joints[:, :, 1] += np.tile(np.linspace(-0.45, 0.45, persons) if persons > 1 else [0.0], FRAMES)[:, None]
        where = np.repeat(np.arange(FRAMES), persons)

        def chunk():
            panel.fill_(255)
            m.render_segments(panel, grid, grid_segments, [pipe.GRID_COLOUR] * len(grid_segments), [grid_w] * len(grid_segments), list(range(FRAMES)))
            m.render_segments(panel, joints, bones, colours, [bone_w] * len(bones), where, R=R)

        ms = events(chunk)
        covered = int((panel != 255).any(-1).sum().item()) // FRAMES
        mpl = matplotlib_seconds(pipe, joints[0].astype(np.float64), np) if persons == 1 else None
        lines.append(f"{persons} {ms:.4f} {ms / FRAMES:.4f} {covered} {'-' if mpl is None else f'{mpl:.4f}'}")
        print(lines[-1], flush=True)
    m.close()
    argv = sys.argv[1:]
    with open(argv[0] if argv else os.path.join(root, "profiles", "skeleton_times.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    signal.alarm(0)


if __name__ == "__main__":
    main()
