"""Host side of the renderer (csrc/ses_render.hip): the palette, palette indices -> RGB, and GIF files.

The device produces palette-indexed frames (HipES.render: uint8[n, H, W], indices 0 .. 15); nothing here touches the device, so
the module imports without one.  PALETTE repeats the 48 bytes of csrc/ses_render.h (ses_render_palette); tests/test_gpu_render.py
holds the two equal.
"""
import numpy as np

PALETTE = np.array([
    (0, 0, 0),          # 0  black: CartPole's cart and track, the walker's flag pole, LunarLander's sky
    (255, 255, 255),    # 1  white: CartPole's and simple_spread's background, the moon, the helipad poles
    (230, 230, 255),    # 2  sky: BipedalWalker's background
    (102, 153, 76),     # 3  grass: BipedalWalker's terrain
    (255, 0, 0),        # 4  red: the lidar rays
    (204, 204, 0),      # 5  yellow: the helipad flags
    (127, 102, 230),    # 6  hull: the lander's and the walker's hull
    (77, 77, 128),      # 7  the lander's legs
    (204, 153, 102),    # 8  CartPole's pole
    (127, 127, 204),    # 9  CartPole's axle
    (178, 102, 153),    # 10 the walker's leg -1
    (127, 51, 102),     # 11 the walker's leg +1
    (64, 64, 64),       # 12 simple_spread's landmarks
    (89, 89, 217),      # 13 simple_spread's agents
    (128, 128, 128),    # 14 grey (no scene uses it)
    (230, 51, 0),       # 15 the walker's start flag
], dtype=np.uint8)


def palette():
    """uint8[16, 3]: the RGB triple of every palette index."""
    return PALETTE.copy()


def to_rgb(frames):
    """palette-indexed frames uint8[..., H, W] (numpy, or a torch tensor on any device) -> RGB uint8[..., H, W, 3]."""
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    return PALETTE[np.asarray(frames, dtype=np.uint8) & 15]


def write_gif(path, frames, fps=30):
    """Write palette-indexed frames uint8[n, H, W] as an animated GIF that carries the 16-colour palette itself."""
    try:
        from PIL import GifImagePlugin, Image
    except ImportError as e:
        raise RuntimeError("write_gif needs PIL (pillow) to encode GIF files, and it cannot be imported here") from e
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    frames = np.ascontiguousarray(frames, dtype=np.uint8) & 15
    if frames.ndim != 3 or frames.shape[0] < 1:
        raise ValueError(f"write_gif: expected frames [n >= 1, H, W], got {frames.shape}")
    flat = PALETTE.reshape(-1).tolist() + [0] * (768 - 48)
    images = []
    height, width = frames.shape[1:]
    for f in frames:
        im = Image.frombytes("P", (width, height), f.tobytes())
        im.putpalette(flat)
        images.append(im)
    # One image block per frame through PIL's own header / frame encoders.  (Image.save(save_all=True) merges a frame that equals
    # its predecessor into it; a playback of T steps has T frames, also while nothing moves.)
    duration = max(10, int(round(1000.0 / fps)))                 # GIF counts in 1/100 s
    header, _ = GifImagePlugin.getheader(images[0], info={"loop": 0})
    with open(path, "wb") as fp:
        for chunk in header:
            fp.write(chunk)
        for im in images:
            for chunk in GifImagePlugin.getdata(im, duration=duration, disposal=1):
                fp.write(chunk)
        fp.write(b";")
