"""Rendering of a triangle mesh on the device, in place of the OpenGL passes of utils/hodan_renderer.py.
Depth: what the reference's vsd() calls as render(model, im_size, K, R, t, clip_near=100, clip_far=10000, mode='depth')
(utils/pose_error.py:124-128).  Pixel (r, c) holds the camera-frame Z of the nearest surface point through (c + 0.5, r + 0.5)
in OpenCV pixel coordinates, 0 where the mesh does not cover it (csrc/render.hip).  render() has only mode='depth'.
Colour: render_rgbd_batch / render_object give the renderer's 'rgb' and 'rgb+depth' modes (flat or phong shaded, :22-103,
:309-352, :473-518): vertex colours from pp_render_rgbd, and a UV-mapped model with its texture image (texture= or
model['texture'], with model['texture_uv']: utils.ply_loader.load_ply(path, texture=True)) from pp_render_rgbd_tex, as the
shaders' texture branch does (:56-57, 72-76, 98-102).  The texture is sampled without mip-maps, tex_filter 'nearest' |
'bilinear' and tex_wrap 'clamp' | 'repeat'; the defaults, nearest and clamp, are our reading of glumpy's texture object, which is
unpinned.  light_cam_pos is given in the OpenCV camera frame; the defaults ambient_weight=0.5 and a light at the camera origin
are those of bop_toolkit's renderer base class, which is not part of the reference checkout; parity with an OpenGL driver is
unpinned (tests/render_rgb_np.py restates the shading rule, tests/render_tex_np.py the sampling rule)."""
import numpy as np
import torch

from .. import ops
from ..runtime import default_context
from ._host import k4, to_device


def _mesh(model):
    pts = np.asarray(model["pts"], np.float64)
    faces = np.asarray(model["faces"])
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError("model['pts'] must be n x 3")
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError("model['faces'] must be m x 3 (triangles only)")
    fi = faces.astype(np.int64)
    if not np.array_equal(fi, faces) or fi.min() < 0 or fi.max() >= pts.shape[0]:
        raise ValueError("model['faces'] must hold vertex indices in [0, %d)" % pts.shape[0])
    return pts, fi.astype(np.int32)


def render_depth_batch(model, im_size, K, R, t, clip_near=100, clip_far=10000, ctx=None):
    """n poses of one mesh in one launch: model dict ('pts' [n_v,3], 'faces' [n_f,3]), im_size (w, h), K 3x3 or [n,3,3],
    R [n,3,3], t [n,3] (the unit of pts) -> cuda float32 tensor [n, h, w]."""
    w, h = (int(v) for v in im_size)
    pts, faces = _mesh(model)
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    n = R.shape[0]
    return ops.render_depth(ctx or default_context(), to_device(pts), to_device(faces, torch.int32), to_device(R), to_device(t, shape=(n, 3)),
                            to_device(k4(K, n)), w, h, float(clip_near), float(clip_far))


def render(model, im_size, K, R, t, clip_near=100, clip_far=10000, mode="depth", ambient_weight=0.5, surf_color=None,
           shading="phong"):
    """One depth image [h, w] float32 (numpy), im_size = (w, h); the signature vsd() calls.  The colour arguments of the
    reference's renderer are accepted for signature compatibility and must stay at their defaults: RGB is not rendered."""
    if mode != "depth":
        raise ValueError("render: only mode='depth' is implemented (got %r)" % (mode,))
    return render_depth_batch(model, im_size, K, R, t, clip_near, clip_far)[0].cpu().numpy()


RGBD_OUTPUTS = ("rgb", "rgb_f32", "depth", "tri_id")


def _colors(model, n_vert, surf_color):
    """vertex colours as hodan_renderer.py:309-352 picks them: surf_color, else model['colors'] (divided by 255 when its
    maximum exceeds 1), else grey 0.5 -> float64 [n_vert,3] in [0, 1]"""
    if surf_color is not None:
        c = np.asarray(surf_color, np.float64).reshape(-1)
        if c.size != 3:
            raise ValueError("surf_color must hold 3 values, got %d" % c.size)
        colors = np.tile(c, (n_vert, 1))
    elif "texture_file" in model:
        raise ValueError("render_rgbd_batch: the model names a texture file but carries no image: load it with "
                         "load_ply(path, texture=True), pass texture=, or give surf_color")
    elif "colors" in model:
        colors = np.array(model["colors"], np.float64)
        if colors.ndim != 2 or colors.shape[0] != n_vert or colors.shape[1] < 3:
            raise ValueError("model['colors'] must be %d x 3, got %s" % (n_vert, colors.shape))
        colors = colors[:, :3]
        if colors.size and colors.max() > 1.0:
            colors = colors / 255.0
    else:
        colors = np.full((n_vert, 3), 0.5)
    if not (np.isfinite(colors).all() and colors.min() >= 0.0 and colors.max() <= 1.0):
        raise ValueError("vertex colours must lie in [0, 1] (or in [0, 255])")
    return np.ascontiguousarray(colors)


def texture_rgbx(texture):
    """a texture image [h,w,3] or [h,w,4] -- uint8 (numpy or a tensor), or float in [0, 1] whose values are k / 255, converted
    exactly -> cuda uint8 tensor [h,w,4] (RGBX), what ops.render_rgbd_tex takes.  A float image off the 1/255 grid is refused.
    A contiguous cuda uint8 [h,w,4] tensor comes back as it is: a caller that renders many batches or scenes of one model
    converts once (model['texture'] = texture_rgbx(image)) instead of padding and uploading the host image on every call."""
    if torch.is_tensor(texture):
        if texture.dtype != torch.uint8:
            raise ValueError("texture: a tensor must be uint8, got %s" % str(texture.dtype)[6:])
        a = texture
    else:
        a = np.asarray(texture)
    if a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("texture must be [h,w,3] or [h,w,4], got %s" % (tuple(a.shape),))
    if not torch.is_tensor(a) and a.dtype != np.uint8:
        if a.dtype.kind != "f":
            raise ValueError("texture must be uint8, or float in [0, 1], got %s" % a.dtype)
        with np.errstate(invalid="ignore"):
            k = np.rint(a.astype(np.float64) * 255.0)
            on_grid = (k >= 0) & (k <= 255) & ((a == (k / 255.0).astype(a.dtype)) | (a == k.astype(a.dtype) / a.dtype.type(255)))
        if not on_grid.all():
            raise ValueError("texture: a float image must hold values k / 255 in [0, 1] (give uint8 otherwise: nothing is rounded)")
        a = k.astype(np.uint8)
    if a.shape[2] == 3:  # pad to one 32-bit word per texel
        if torch.is_tensor(a):
            a = torch.cat([a, torch.full_like(a[..., :1], 255)], dim=2)
        else:
            a = np.concatenate([a, np.full(a.shape[:2] + (1,), 255, np.uint8)], axis=2)
    return to_device(a, torch.uint8)


def _texture(model, n_vert, surf_color, texture):
    """(uv float64 [n_vert,2], the texture as texture_rgbx gives it) when the model is drawn textured -- no surf_color and an
    image at hand, texture or else model['texture'] -- or None"""
    image = texture if texture is not None else model.get("texture")
    if surf_color is not None or image is None:
        return None
    if model.get("texture_uv") is None:
        raise ValueError("render_rgbd_batch: a textured model needs model['texture_uv'] [%d,2]" % n_vert)
    uv = np.asarray(model["texture_uv"], np.float64)
    if uv.shape != (n_vert, 2) or not np.isfinite(uv).all():
        raise ValueError("model['texture_uv'] must be %d x 2 and finite, got %s" % (n_vert, uv.shape))
    return np.ascontiguousarray(uv), texture_rgbx(image)


def render_rgbd_batch(model, im_size, K, R, t, clip_near=100, clip_far=10000, shading="phong", ambient_weight=0.5,
                      light_cam_pos=(0, 0, 0), surf_color=None, bg_color=(0, 0, 0), outputs=("rgb", "depth"), ctx=None, texture=None,
                      tex_filter="nearest", tex_wrap="clamp"):
    """n poses of one mesh in one launch: model dict ('pts', 'faces', optionally 'colors' [n_v,3] and 'normals' [n_v,3]),
    im_size (w, h), K 3x3 or [n,3,3], R [n,3,3], t [n,3]; shading 'phong' (needs model['normals']) or 'flat'; light_cam_pos in
    the OpenCV camera frame; outputs: any of 'rgb' (uint8 [n,h,w,3], RGB), 'rgb_f32' (float32), 'depth' (float32 [n,h,w]),
    'tri_id' (int32 [n,h,w], -1 = none) -> dict of cuda tensors.
    Without surf_color, a model with a texture image -- texture, else model['texture']: [h,w,3] or [h,w,4], uint8 (numpy or
    tensor) or float values k / 255, rows as in the image file -- is drawn textured through model['texture_uv'] [n_v,2] (v = 0
    is the image's bottom row); tex_filter 'nearest' | 'bilinear', tex_wrap 'clamp' | 'repeat'.  A host image is padded and
    uploaded on every call: for repeated calls keep texture_rgbx(image), a cuda tensor, in its place."""
    w, h = (int(v) for v in im_size)
    pts, faces = _mesh(model)
    if shading not in ops.RENDER_SHADING:
        raise ValueError("render_rgbd_batch: unknown shading %r (flat | phong)" % (shading,))
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outputs or any(o not in RGBD_OUTPUTS for o in outputs):
        raise ValueError("render_rgbd_batch: outputs must name at least one of %s, got %r" % (" | ".join(RGBD_OUTPUTS), outputs))
    if tex_filter not in ops.RENDER_FILTER:
        raise ValueError("render_rgbd_batch: unknown tex_filter %r (nearest | bilinear)" % (tex_filter,))
    if tex_wrap not in ops.RENDER_WRAP:
        raise ValueError("render_rgbd_batch: unknown tex_wrap %r (clamp | repeat)" % (tex_wrap,))
    colors = normals = textured = None
    if any(o.startswith("rgb") for o in outputs):
        textured = _texture(model, pts.shape[0], surf_color, texture)
        if textured is None:
            colors = _colors(model, pts.shape[0], surf_color)
        if shading == "phong":
            if model.get("normals") is None:
                raise ValueError("render_rgbd_batch: shading='phong' needs model['normals'] (use shading='flat' without them)")
            normals = np.asarray(model["normals"], np.float64)
            if normals.shape != pts.shape:
                raise ValueError("model['normals'] must be %d x 3, got %s" % (pts.shape[0], normals.shape))
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    n = R.shape[0]
    dev = lambda a: None if a is None else to_device(a)
    if textured is not None:
        return ops.render_rgbd_tex(ctx or default_context(), to_device(pts), to_device(faces, torch.int32), to_device(R),
                                   to_device(t, shape=(n, 3)), to_device(k4(K, n)), w, h, to_device(textured[0]), textured[1], tex_filter,
                                   tex_wrap, dev(normals), float(clip_near), float(clip_far), shading, float(ambient_weight),
                                   light_cam_pos, bg_color, outputs)
    return ops.render_rgbd(ctx or default_context(), to_device(pts), to_device(faces, torch.int32), to_device(R), to_device(t, shape=(n, 3)),
                           to_device(k4(K, n)), w, h, dev(colors), dev(normals), float(clip_near), float(clip_far), shading,
                           float(ambient_weight), light_cam_pos, bg_color, outputs)


RENDER_MODES = {"rgb": ("rgb",), "depth": ("depth",), "rgb+depth": ("rgb", "depth")}


def render_object(model, im_size, K, R, t, mode="rgb+depth", clip_near=100, clip_far=10000, shading="phong", ambient_weight=0.5,
                  light_cam_pos=(0, 0, 0), surf_color=None, bg_color=(0, 0, 0), texture=None, tex_filter="nearest", tex_wrap="clamp"):
    """One pose of one mesh, as the reference's RendererPython.render_object returns it for the renderer's mode
    (hodan_renderer.py:473-478): {'rgb': uint8 [h,w,3]} | {'depth': float32 [h,w]} | both, numpy arrays.  texture, tex_filter,
    tex_wrap: see render_rgbd_batch."""
    if mode not in RENDER_MODES:
        raise ValueError("render_object: unknown mode %r (rgb | depth | rgb+depth)" % (mode,))
    out = render_rgbd_batch(model, im_size, K, np.asarray(R, np.float64).reshape(1, 3, 3), np.asarray(t, np.float64).reshape(1, 3),
                            clip_near, clip_far, shading, ambient_weight, light_cam_pos, surf_color, bg_color, RENDER_MODES[mode],
                            texture=texture, tex_filter=tex_filter, tex_wrap=tex_wrap)
    return {k: v[0].cpu().numpy() for k, v in out.items()}
