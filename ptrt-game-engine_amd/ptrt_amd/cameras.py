"""Ray generators for Scene.query_radiance: cameras the path tracer's own pinhole / thin lens cannot be.  Pure torch -- the
rays are ordinary tensors, made on whatever device the caller names and handed to the query in place."""
import math


def equirect_rays(width, height, origin=(0.0, 0.0, 0.0), device="cpu"):
    """A 360-degree panorama camera at `origin`: (origins, directions), each a contiguous (height * width, 3) float32 tensor
    on `device`, ray y * width + x through the centre of pixel (x, y) of an equirectangular image.  Row 0 looks up (+Y), the
    last row down; along a row the azimuth atan2(d.z, d.x) runs from -pi to pi with x.  The mapping is the inverse of the
    environment-map lookup of the sky (u = (atan2(d.z, d.x) + pi) / 2 pi, v = acos(d.y) / pi): pixel (x, y) looks at the map's
    texel ((x + 0.5) / width, (y + 0.5) / height).  Directions have unit length."""
    import torch
    w, h = int(width), int(height)
    if w < 1 or h < 1:
        raise ValueError(f"equirect_rays: {w}x{h} image")
    dev = torch.device(device)
    # angles in float64, rounded once: the directions are unit vectors to float32 precision
    theta = (torch.arange(h, dtype=torch.float64, device=dev) + 0.5) * (math.pi / h)
    phi = (torch.arange(w, dtype=torch.float64, device=dev) + 0.5) * (2.0 * math.pi / w) - math.pi
    st, ct = torch.sin(theta)[:, None], torch.cos(theta)[:, None]
    d = torch.stack([st * torch.cos(phi)[None, :], ct.expand(h, w), st * torch.sin(phi)[None, :]], dim=-1)
    d = (d / d.norm(dim=-1, keepdim=True)).to(torch.float32).reshape(h * w, 3).contiguous()
    o = torch.tensor([float(a) for a in origin], dtype=torch.float32, device=dev).reshape(1, 3).expand(h * w, 3).contiguous()
    return o, d
