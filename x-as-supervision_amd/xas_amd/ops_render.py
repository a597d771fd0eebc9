"""Mesh rasteriser on the device (csrc/render.hip, xas_mesh_render): projected vertices + faces -> flat-shaded image, mask,
z-buffer and face ids.  Forward only; nothing here keeps state between calls or synchronises with the host.  No reference
counterpart: the reference reads its pseudo-images from disk."""
import torch

from xas_amd._lib import call, ptr, query

OUTPUTS = ('img', 'mask', 'zbuf', 'face_id')

# one colour per SMPL body part (the 24 joints of the kinematic tree, smpl_layer.KINTREE_PARENTS order): fixed, so that a
# part keeps its colour from run to run and between processes
PART_PALETTE = (
    (0.90, 0.10, 0.10), (0.10, 0.60, 0.90), (0.95, 0.75, 0.10), (0.55, 0.20, 0.80), (0.10, 0.80, 0.40), (0.95, 0.45, 0.10),
    (0.30, 0.30, 0.95), (0.60, 0.90, 0.15), (0.90, 0.20, 0.60), (0.15, 0.85, 0.85), (0.70, 0.45, 0.20), (0.45, 0.70, 0.95),
    (0.95, 0.60, 0.70), (0.20, 0.50, 0.25), (0.75, 0.75, 0.30), (0.50, 0.10, 0.30), (0.35, 0.95, 0.65), (0.80, 0.35, 0.95),
    (0.25, 0.25, 0.55), (0.95, 0.90, 0.55), (0.60, 0.60, 0.60), (0.85, 0.55, 0.40), (0.40, 0.85, 0.95), (0.65, 0.15, 0.10))


def part_colours(skin_weights, faces):
    """[F,3] float32: every face takes the palette colour of the body part of its FIRST vertex, the part being the argmax of
    that vertex's skinning weights (skin_weights [Nv,24], SMPL_Layer.th_weights; faces [F,3])."""
    if skin_weights.dim() != 2 or skin_weights.shape[1] > len(PART_PALETTE):
        raise RuntimeError('part_colours: skin_weights must be [Nv, parts <= %d]' % len(PART_PALETTE))
    part = skin_weights.argmax(dim=1)[faces[:, 0].long()]
    return torch.tensor(PART_PALETTE, dtype=torch.float32, device=skin_weights.device)[part]


def render_mesh(verts, faces, face_rgb=None, light=None, ambient=0.35, depth_scale=1.0, background=0.0, size=256,
                want=('img', 'mask')):
    """verts [B,Nv,3] = (x px, y px, depth) in the patch, faces [F,3] integer -> dict of the outputs named in `want`:
    img [B,3,S,S], mask [B,1,S,S] (1 / 0), zbuf [B,S,S] (+inf where nothing was hit), face_id [B,S,S] int32 (-1 likewise).
    face_rgb [F,3] in [0,1] or None = white; light: a device tensor [3] (the direction towards the light in (x, y, depth *
    depth_scale) space) or None = (0, 0, -1), from the viewer.  The semantics are those of include/xas_hip.h."""
    unknown = set(want) - set(OUTPUTS)
    if unknown:
        raise ValueError('render_mesh: unknown outputs %s (known: %s)' % (sorted(unknown), ', '.join(OUTPUTS)))
    if verts.dim() != 3 or verts.shape[-1] != 3 or faces.dim() != 2 or faces.shape[-1] != 3:
        raise RuntimeError('render_mesh: verts must be [B,Nv,3] and faces [F,3]')
    verts = verts.detach().float().contiguous()
    faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
    B, Nv, F, S = verts.shape[0], verts.shape[1], faces.shape[0], int(size)
    if face_rgb is not None:
        if tuple(face_rgb.shape) != (F, 3):
            raise RuntimeError('render_mesh: face_rgb must be [F,3]')
        face_rgb = face_rgb.to(device=verts.device, dtype=torch.float32).contiguous()
    if light is not None:
        if not torch.is_tensor(light) or light.numel() != 3:
            raise RuntimeError('render_mesh: light must be a tensor of 3 elements')
        light = light.to(device=verts.device, dtype=torch.float32).contiguous()
    dev = verts.device
    img = torch.empty(B, 3, S, S, device=dev, dtype=torch.float32)
    mask = torch.empty(B, 1, S, S, device=dev, dtype=torch.float32)
    zbuf = torch.empty(B, S, S, device=dev, dtype=torch.float32) if 'zbuf' in want else None
    fid = torch.empty(B, S, S, device=dev, dtype=torch.int32) if 'face_id' in want else None
    nbytes = query('xas_mesh_render_workspace_bytes', B, F, S)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    call('xas_mesh_render', ptr(verts), ptr(faces), ptr(face_rgb), ptr(light), float(ambient), float(depth_scale),
         float(background), B, Nv, F, S, ptr(img), ptr(mask), ptr(zbuf), ptr(fid), ptr(ws))
    out = {'img': img, 'mask': mask, 'zbuf': zbuf, 'face_id': fid}
    return {k: out[k] for k in OUTPUTS if k in want}
