"""Device-time cost of the input path, before and after DeviceAugment, at
32 px and 224 px, batch 64.

today  : fp32 NCHW batch -> device-to-device copy into the static buffer,
         then what NativeResNet.forward does to it inside the step:
         permute(0, 2, 3, 1).contiguous() and .to(bfloat16)   (3 launches)
ingest : uint8 NHWC batch -> device-to-device copy into the static buffer,
         then image_ingest + the counter bump                  (3 launches)
h2d    : pinned host -> device copy of the fp32 and of the uint8 batch
kernel : k_image_ingest alone; bytes/s = (3 B read + 6 B written per
         output pixel) / time

today, ingest and kernel are each captured into a HIP graph of 20
repetitions and the replay is timed, as the step itself runs from a graph:
the figure is device time per repetition, without host launch cost.  The
host-to-device copies are timed eagerly.  Every figure comes from device
events around back-to-back calls after a warmup; the cases alternate over
`rounds` rounds and the table gives the median with the min..max spread.
The repeated buffers stay resident in the 256 MiB Infinity Cache, as they
largely do in a real step (the batch was just written by the prefetch copy).

A second table times the random resized crop at 256 x (256x256 -> 224x224),
the ImageNet training shape, on pre-resized storage:

resized : DeviceResizedCrop as called: k_resized_crop_draw + k_resized_crop
          + the counter bump                                   (3 launches)
resample: k_resized_crop alone on the boxes of the last draw
draw    : k_resized_crop_draw + the counter bump alone        (2 launches)
crop    : k_image_ingest (translate-only crop) at the same shapes, + bump
eager   : what the kernel replaces: per sample, slice the box, F.interpolate
          (bilinear) to 224x224, flip, normalize, cast and write NHWC, with
          boxes fixed on the host.  It cannot vary under graph replay, so it
          is timed eagerly (device events around the enqueued calls): the
          figure includes the launch gaps of its ~1700 small kernels, which
          is the cost a user of that path pays.

resized, resample, draw and crop are graph-captured like the first table's cases.
Bytes for the resample: the compulsory traffic is each sample's box read
once (h * w * 3 B, summed over the drawn boxes) plus 6 B written per output
pixel; the gathers themselves issue 4 taps x 3 B per output pixel, most of
which L2 serves.  GB/s is compulsory bytes over the resample's time.

--json writes {"ingest": [the two rows of the first table], "resized_crop":
{the second table}}; before the second table existed it wrote the bare list
of rows.

Run on a GPU:  PYTHONPATH=. python scripts/ingest_cost.py [--json out.json]
"""
import argparse
import json
import math
import statistics

import torch

import flashy_amd.ops as ops
from flashy_amd.data import DeviceAugment, DeviceResizedCrop

BATCH = 64
RC_BATCH, RC_SRC, RC_OUT = 256, 256, 224
REPS = 20
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn, iters):
    """Mean device microseconds of one fn() over `iters` enqueued calls."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def graphed(fn):
    """fn repeated REPS times in one captured graph; returns its replay."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(REPS):
            fn()
    return graph.replay


def measure(size, pad, iters, rounds):
    src_px = size + 2 * 16 if size > 32 else size   # 224 from 256, 32 pad 4
    f32_host = torch.randn(BATCH, 3, size, size).pin_memory()
    u8_host = torch.randint(0, 256, (BATCH, src_px, src_px, 3),
                            dtype=torch.uint8).pin_memory()
    f32_dev, u8_dev = f32_host.cuda(), u8_host.cuda()
    static_f32 = torch.empty_like(f32_dev)
    static_u8 = torch.empty_like(u8_dev)
    static_out = torch.empty(BATCH, size, size, 3, dtype=torch.bfloat16,
                             device="cuda")
    h2d_f32 = torch.empty_like(f32_dev)
    h2d_u8 = torch.empty_like(u8_dev)
    aug = DeviceAugment(size, pad=pad, mean=MEAN, std=STD)

    def today():
        static_f32.copy_(f32_dev, non_blocking=True)
        x = static_f32.permute(0, 2, 3, 1).contiguous()
        return x.to(torch.bfloat16)

    def ingest():
        static_u8.copy_(u8_dev, non_blocking=True)
        return aug(static_u8, out=static_out)

    ext = ops.require()
    thresh = round(aug.flip * 2 ** 24)

    def kernel_only():
        ext.image_ingest(static_u8.data_ptr(), static_out.data_ptr(),
                         aug._step_dev.data_ptr(), BATCH, src_px, src_px,
                         size, size, pad, aug.seed, thresh, list(aug.scale),
                         list(aug.bias), aug.fill, True,
                         torch.cuda.current_stream().cuda_stream)

    graphs = {"today_us": graphed(today), "ingest_us": graphed(ingest),
              "kernel_us": graphed(kernel_only)}
    copies = {
        "h2d_f32_us": lambda: h2d_f32.copy_(f32_host, non_blocking=True),
        "h2d_u8_us": lambda: h2d_u8.copy_(u8_host, non_blocking=True),
    }
    samples = {k: [] for k in (*graphs, *copies)}
    for _ in range(rounds):
        for name, replay in graphs.items():
            samples[name].append(timed(replay, iters) / REPS)
        for name, fn in copies.items():
            samples[name].append(timed(fn, iters))

    row = {"size": size, "src_px": src_px, "pad": pad, "batch": BATCH}
    for name, vals in samples.items():
        row[name] = {"median": statistics.median(vals), "min": min(vals),
                     "max": max(vals)}
    out_px = BATCH * size * size
    row["kernel_bytes"] = out_px * (3 + 6)
    row["kernel_tb_per_s"] = row["kernel_bytes"] / \
        (row["kernel_us"]["median"] * 1e-6) / 1e12
    row["today_bytes"] = out_px * 3 * (4 + 4 + 4 + 4 + 4 + 2)
    row["ingest_bytes"] = u8_dev.numel() * 2 + out_px * (3 + 6)
    return row


def _summary(samples):
    return {name: {"median": statistics.median(vals), "min": min(vals),
                   "max": max(vals)} for name, vals in samples.items()}


def measure_resized(iters, rounds):
    from torch.nn import functional as F
    n, src_px, size = RC_BATCH, RC_SRC, RC_OUT
    u8 = torch.randint(0, 256, (n, src_px, src_px, 3), dtype=torch.uint8,
                       device="cuda")
    out = torch.empty(n, size, size, 3, dtype=torch.bfloat16, device="cuda")
    rc = DeviceResizedCrop(size, mean=MEAN, std=STD)
    crop = DeviceAugment(size, pad=0, mean=MEAN, std=STD)
    ext = ops.require()

    def resized():
        return rc(u8, out=out)

    def crop_only():
        return crop(u8, out=out)

    resized()
    # a private copy: the resample and the eager chain keep working on these
    # boxes while the other cases draw new ones into the augment's buffer
    boxes_dev = rc.last_boxes.clone()
    draw_dev = rc.last_boxes
    box_bytes = int((boxes_dev[:, 2].long() * boxes_dev[:, 3].long()).sum()) * 3

    def resample_only():
        ext.resized_crop(u8.data_ptr(), out.data_ptr(), boxes_dev.data_ptr(),
                         n, src_px, src_px, size, size, list(rc.scale),
                         list(rc.bias),
                         torch.cuda.current_stream().cuda_stream)

    thresh, r0, r1, crop_q16 = rc._consts()
    root = math.isqrt((src_px * src_px) << 32)

    def draw_only():
        stream = torch.cuda.current_stream().cuda_stream
        ext.resized_crop_draw(draw_dev.data_ptr(), rc._tables_dev.data_ptr(),
                              rc._step_dev.data_ptr(), n, src_px, src_px,
                              size, size, rc.seed, root, thresh, r0, r1,
                              crop_q16, True, stream)
        ext.adam_step_inc(rc._step_dev.data_ptr(), stream)

    boxes = boxes_dev.cpu().tolist()
    scale = torch.tensor(rc.scale, device="cuda").view(1, 3, 1, 1) * 255.0
    bias = torch.tensor(rc.bias, device="cuda").view(1, 3, 1, 1)

    def eager():
        for i, (y0, x0, h, w, flip, *_) in enumerate(boxes):
            box = u8[i, y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None]
            img = F.interpolate(box.float() / 255.0, size=(size, size),
                                mode="bilinear", align_corners=False)
            if flip:
                img = img.flip(3)
            out[i].copy_((img * scale + bias)[0].permute(1, 2, 0))
        return out

    graphs = {"resized_us": graphed(resized),
              "resample_us": graphed(resample_only),
              "draw_us": graphed(draw_only),
              "crop_us": graphed(crop_only)}
    samples = {k: [] for k in (*graphs, "eager_us")}
    for _ in range(rounds):
        for name, replay in graphs.items():
            samples[name].append(timed(replay, iters) / REPS)
        samples["eager_us"].append(timed(eager, max(1, iters // 20)))
    row = {"batch": n, "src_px": src_px, "size": size, **_summary(samples)}
    out_px = n * size * size
    row["resample_bytes"] = box_bytes + out_px * 6
    row["resample_gather_bytes"] = out_px * (12 + 6)
    row["resample_gb_per_s"] = row["resample_bytes"] / \
        (row["resample_us"]["median"] * 1e-6) / 1e9
    row["crop_bytes"] = out_px * (3 + 6)
    row["crop_gb_per_s"] = row["crop_bytes"] / \
        (row["crop_us"]["median"] * 1e-6) / 1e9
    return row


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--iters", type=int, default=200)
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--json", default=None)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: device times only"
    rows = [measure(32, 4, args.iters, args.rounds),
            measure(224, 0, args.iters, args.rounds)]
    for row in rows:
        print(f"--- {row['size']} px from {row['src_px']} px, pad "
              f"{row['pad']}, batch {row['batch']}")
        for name in ("today_us", "ingest_us", "h2d_f32_us", "h2d_u8_us",
                     "kernel_us"):
            v = row[name]
            print(f"{name:>12}: {v['median']:9.2f} us  "
                  f"({v['min']:.2f} .. {v['max']:.2f})")
        print(f"{'kernel':>12}: {row['kernel_bytes'] / 1e6:.2f} MB -> "
              f"{row['kernel_tb_per_s']:.3f} TB/s")
    rc = measure_resized(args.iters, args.rounds)
    print(f"--- resized crop: {rc['batch']} x ({rc['src_px']} px -> "
          f"{rc['size']} px)")
    for name in ("resized_us", "resample_us", "draw_us", "crop_us",
                 "eager_us"):
        v = rc[name]
        print(f"{name:>12}: {v['median']:9.2f} us  "
              f"({v['min']:.2f} .. {v['max']:.2f})")
    print(f"{'resample':>12}: {rc['resample_bytes'] / 1e6:.2f} MB compulsory "
          f"({rc['resample_gather_bytes'] / 1e6:.2f} MB gathered) -> "
          f"{rc['resample_gb_per_s']:.0f} GB/s")
    print(f"{'crop':>12}: {rc['crop_bytes'] / 1e6:.2f} MB -> "
          f"{rc['crop_gb_per_s']:.0f} GB/s")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"ingest": rows, "resized_crop": rc}, fh, indent=1)


if __name__ == "__main__":
    main()
