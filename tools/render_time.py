"""Time of the mesh overlay (GRNet.render = grnet_render_meshes) next to the forward, by HIP events, on one MI355X:

    render_ms_per_frame   one GRNet.render call over F frames of 1920 x 1080 resident on the device, P persons per frame (P = 1, 4), main view,
                          divided by F; the meshes are the forward's own vertices for synthetic frames, scaled into the picture
    forward_ms_per_frame  model(frames) at the same call size F, divided by F
    wireframe_ms_per_frame, wireframe_pixels_per_frame (--wireframe only)
                          the same call with wireframe=True (demo.py --wireframe), measured in the same run next to the filled overlay
Medians of REPS runs after a warm one.  No bar: the renderer has no predecessor and the reference's cannot run here.

    python tools/render_time.py [--wireframe] [path]        writes the file whole; default: profiles/render_times.txt
"""
import importlib
import os
import statistics
import sys

REPS = 10
FRAMES = 16
H, W = 1080, 1920


def main():
    argv = [a for a in sys.argv[1:] if a != "--wireframe"]
    wireframe = "--wireframe" in sys.argv[1:]
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    assert torch.cuda.is_available(), "render_time.py measures on the GPU; there is no CPU figure to report"
    m = pkg.build_synthetic_model(max_frames=FRAMES, with_gru=False, compact_arena=True)
    frames = torch.from_numpy(pkg.synth.make_frames(FRAMES)).cuda().unsqueeze(0)

    def events(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            keep = fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
            del keep
        return statistics.median(ts)

    verts = m(frames)[-1]["verts"].reshape(FRAMES, 6890, 3).clone()
    forward_ms = events(lambda: m(frames)) / FRAMES
    images = torch.zeros(FRAMES, H, W, 3, dtype=torch.uint8, device="cuda")
    lines = [f"# the mesh overlay on one MI355X: {FRAMES} frames of {W} x {H} per call, images on the device, synthetic meshes (a tangle of 13 780 triangles",
             "# about 600 pixels tall per person); ms per frame, medians of HIP-event times (tools/render_time.py)",
             "# persons render_ms_per_frame forward_ms_per_frame covered_pixels_per_frame" + (" wireframe_ms_per_frame wireframe_pixels_per_frame" if wireframe else "")]
    for persons in (1, 4):
        idx = np.repeat(np.arange(FRAMES), persons)
        v = verts[idx]
        cams = np.stack([(0.5 * H / W, 0.5, 0.6 * (k % persons) - 0.3 * (persons - 1), 0.0) for k in range(len(idx))]).astype(np.float32)
        cols = np.full((len(idx), 3), 0.8, np.float32)
        images.zero_()
        m.render(images, v, cams, cols, idx)
        covered = int((images != 0).any(-1).sum().item()) // FRAMES
        ms = events(lambda: m.render(images, v, cams, cols, idx)) / FRAMES
        lines.append(f"{persons} {ms:.4f} {forward_ms:.4f} {covered}")
        if wireframe:
            images.zero_()
            m.render(images, v, cams, cols, idx, wireframe=True)
            wire_covered = int((images != 0).any(-1).sum().item()) // FRAMES
            wire_ms = events(lambda: m.render(images, v, cams, cols, idx, wireframe=True)) / FRAMES
            lines[-1] += f" {wire_ms:.4f} {wire_covered}"
        print(lines[-1], flush=True)
    m.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(argv[0] if argv else os.path.join(root, "profiles", "render_times.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
