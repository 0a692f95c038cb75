"""Ray generators for Renderer.render_rays (pt_radiance): each returns
(origins (n, 3) f64, dirs (n, 3) f64, keys (n,) u32) in the reference's list
order k = ix*H + iy (x outer, y inner, iy upwards — utils.py:64-69), with
key = k, so `rays_to_image` puts the result into image orientation;
`to_image_order` reorders the rays themselves, for an H x W ray accumulator
(Renderer.render_rays_adaptive with shape=(H, W))."""
import numpy as np


def _list_keys(W, H):
    return np.arange(int(W) * int(H), dtype=np.uint32)


def scene_camera_rays(scene, W=None, H=None):
    """Exactly the frame's rays and keys: o = eye, d = (x - ex, y - ey,
    0 - ez) with x, y from np.linspace over the scene's ortho window (the
    kernels' linspace_at is its arithmetic), key = ix*H + iy.  render_rays of
    these is Renderer.render of the same size."""
    W = int(scene.width if W is None else W)
    H = int(scene.height if H is None else H)
    eye = np.asarray(scene.eye, dtype=np.float64).reshape(3)
    x0, y0, x1, y1 = [float(v) for v in scene.ortho]
    xs, ys = np.linspace(x0, x1, W), np.linspace(y0, y1, H)
    d = np.empty((W, H, 3), dtype=np.float64)
    d[:, :, 0] = (xs - eye[0])[:, None]
    d[:, :, 1] = (ys - eye[1])[None, :]
    d[:, :, 2] = 0.0 - eye[2]
    o = np.broadcast_to(eye, (W * H, 3)).copy()
    return o, d.reshape(W * H, 3), _list_keys(W, H)


def _basis(eye, target, up):
    eye, target, up = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    f = target - eye
    nf = np.linalg.norm(f)
    if not nf > 0:
        raise ValueError("look-at: eye and target coincide")
    f = f / nf
    r = np.cross(f, up)
    nr = np.linalg.norm(r)
    if not nr > 0:
        raise ValueError("look-at: up is parallel to the view direction")
    r = r / nr
    return eye, f, r, np.cross(r, f)


def _screen(W, H, half_w, half_h):
    """Pixel-centre offsets (sx (W,), sy (H,)) over [-half, half]."""
    W, H = int(W), int(H)
    sx = ((np.arange(W) + 0.5) / W * 2.0 - 1.0) * half_w
    sy = ((np.arange(H) + 0.5) / H * 2.0 - 1.0) * half_h
    return sx, sy


def look_at_rays(eye, target, up=(0.0, 1.0, 0.0), fov_y=40.0, W=64, H=64):
    """A pinhole at `eye` looking at `target`: vertical field of view fov_y
    degrees, square pixels, `up` towards the top of the image; unit
    directions through the pixel centres."""
    eye, f, r, u = _basis(eye, target, up)
    half_h = np.tan(np.radians(float(fov_y)) / 2.0)
    sx, sy = _screen(W, H, half_h * W / H, half_h)
    d = f[None, None, :] + sx[:, None, None] * r[None, None, :] + sy[None, :, None] * u[None, None, :]
    d = d / np.linalg.norm(d, axis=2, keepdims=True)
    n = int(W) * int(H)
    return np.broadcast_to(eye, (n, 3)).copy(), d.reshape(n, 3), _list_keys(W, H)


def ortho_rays(eye, target, up=(0.0, 1.0, 0.0), width=1.0, height=None, W=64, H=64):
    """An orthographic view: parallel rays along eye -> target whose origins
    cover a width x height window (height None: square pixels) centred on
    `eye` in the plane through it."""
    eye, f, r, u = _basis(eye, target, up)
    height = float(width) * H / W if height is None else float(height)
    sx, sy = _screen(W, H, float(width) / 2.0, height / 2.0)
    o = eye[None, None, :] + sx[:, None, None] * r[None, None, :] + sy[None, :, None] * u[None, None, :]
    n = int(W) * int(H)
    return o.reshape(n, 3), np.broadcast_to(f, (n, 3)).copy(), _list_keys(W, H)


def rays_box(origins):
    """The box (lo, hi) of a set of origins, for Renderer(scene, ray_box=...)."""
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    return o.min(axis=0), o.max(axis=0)


def rays_to_image(values, W, H):
    """A result in the generators' ray order (W*H, c) as an image (H, W, c),
    top row first (render.from_list_order's placement)."""
    v = np.asarray(values)
    return v.reshape(int(W), int(H), -1).transpose(1, 0, 2)[::-1]


def to_image_order(origins, dirs, keys, W, H):
    """The generators' list-order rays (k = ix*H + iy) as image-order records:
    (o, d, keys) with record e = (H-1-iy)*W + ix the ray of list index k, keys
    unchanged per ray — what an H x W ray accumulator takes
    (render_rays_adaptive(..., shape=(H, W))); its (H, W, ...) results are then
    images, top row first, as rays_to_image would place them."""
    W, H = int(W), int(H)
    o = rays_to_image(np.asarray(origins, dtype=np.float64).reshape(W * H, 3), W, H).reshape(W * H, 3)
    d = rays_to_image(np.asarray(dirs, dtype=np.float64).reshape(W * H, 3), W, H).reshape(W * H, 3)
    k = rays_to_image(np.asarray(keys).reshape(W * H, 1), W, H).reshape(W * H)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(k)


def from_image_order(values, W, H):
    """Inverse of to_image_order for any per-record array: image-order values
    (H*W, ...) or (H, W, ...) back into the generators' list order (W*H, ...)."""
    W, H = int(W), int(H)
    v = np.asarray(values)
    tail = v.shape[2:] if v.shape[:2] == (H, W) else v.shape[1:]
    v = v.reshape((H, W) + tail)
    return np.ascontiguousarray(np.swapaxes(v[::-1], 0, 1)).reshape((W * H,) + v.shape[2:])
