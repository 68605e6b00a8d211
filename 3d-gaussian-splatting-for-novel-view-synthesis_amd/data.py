"""On-disk data layout of the reference and Gaussian initialisation from a point cloud ("next" row 4).

Layout (gaussian_splatting/data_loader.py:153-284; written by datasets/prepare_mipnerf360.py:410-431):
    <data_dir>/images/*.{jpg,png,JPG,PNG}   cam_meta.npy (a pickled dict: fx, fy[, cx, cy][, c2w])   poses.npy [K,4,4]
    pointcloud.ply (ASCII, x y z first; a binary little-endian file, with its colours, is read as well)
Functions mirror the reference's names and return values: load_image (:15), load_camera_parameters (:27),
load_point_cloud (:50), GaussianDataset (:153), initialize_gaussians_from_pointcloud (:287).  `write_dataset` produces
the same layout (so a scene can be prepared without the reference's download / COLMAP tooling).  Host-side I/O only.
"""
import json
import pickle
from pathlib import Path

import numpy as np
import torch


def load_image(image_path):
    """[H, W, 3] float32 in [0, 1] (data_loader.py:15-25)."""
    from PIL import Image
    return torch.from_numpy(np.array(Image.open(image_path).convert('RGB'), dtype=np.float32) / 255.0)


def load_image_alpha(image_path):
    """([H, W, 3], [H, W]) float32 in [0, 1]: the colour as load_image gives it and the file's alpha channel, 1.0 everywhere for a
    file without one."""
    from PIL import Image
    im = Image.open(image_path)
    rgb = torch.from_numpy(np.array(im.convert('RGB'), dtype=np.float32) / 255.0)
    if 'A' in im.getbands() or 'transparency' in im.info:
        return rgb, torch.from_numpy(np.array(im.convert('RGBA'), dtype=np.float32)[..., 3] / 255.0)
    return rgb, torch.ones(rgb.shape[:2], dtype=torch.float32)


class _MetaUnpickler(pickle.Unpickler):
    """Unpickler for cam_meta.npy that can only rebuild numpy arrays / scalars / dtypes and plain Python containers:
    a crafted file cannot name any other callable, so loading a dataset directory executes nothing from it."""
    _ALLOWED = {("numpy", "ndarray"), ("numpy", "dtype"),
                ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
                ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
                ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer")}

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"cam_meta.npy may only hold numbers, strings, lists, dicts and numpy arrays; it names {module}.{name}")


def load_camera_parameters(cam_meta_path):
    """The camera dict of the reference's layout (data_loader.py:27-47: fx, fy[, cx, cy][, c2w] ...).  The reference stores it
    as a PICKLED dict inside cam_meta.npy and reads it with allow_pickle=True; here the pickle is read by a restricted
    unpickler (numpy arrays and plain containers only), and a cam_meta.json beside it (write_dataset emits one) is
    preferred when present."""
    path = Path(cam_meta_path)
    js = path.with_suffix('.json')
    if js.exists():
        with open(js) as f:
            return json.load(f)
    with open(path, 'rb') as f:
        version = np.lib.format.read_magic(f)
        _, _, dtype = np.lib.format.read_array_header_1_0(f) if version == (1, 0) else np.lib.format.read_array_header_2_0(f)
        if not dtype.hasobject:
            raise ValueError(f"{path}: expected the reference's pickled dict, found a plain array")
        obj = _MetaUnpickler(f).load()
    return obj.item() if isinstance(obj, np.ndarray) and obj.shape == () else obj


def _filter_points(pts, extra=None):
    """The sanitising of data_loader.py:106-148: drop NaN/Inf, keep |coord| < 1000 if any such point exists, otherwise
    fall back to the 99th-percentile / 100 x median distance filters; an empty result raises ValueError.  `extra` (not in the
    reference): further columns of the same rows (colours), which play no part in the tests; the kept rows come back as [K, 3 + E]."""
    rows = torch.arange(len(pts))

    def keep(mask):
        return pts[mask], rows[mask]

    pts, rows = keep(torch.isfinite(pts).all(dim=1))
    if len(pts) > 0:
        near = (pts.abs() < 1000).all(dim=1)
        if near.sum() > 0:
            pts, rows = keep(near)
        else:
            dist = (pts - pts.mean(dim=0)).norm(dim=1)
            if len(dist) > 100:
                ok = dist < torch.quantile(dist, 0.99)
                if ok.sum() > 0:
                    pts, rows = keep(ok)
                else:
                    med = dist.median()
                    if torch.isfinite(med) and med > 0 and (dist < med * 100).sum() > 0:
                        pts, rows = keep(dist < med * 100)
    if len(pts) == 0:
        raise ValueError("Point cloud is empty after filtering invalid values!")
    return pts if extra is None else torch.cat([pts, extra[rows]], dim=1)


# PLY scalar types -> little-endian numpy types
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': '<i2', 'int16': '<i2', 'ushort': '<u2', 'uint16': '<u2',
              'int': '<i4', 'int32': '<i4', 'uint': '<u4', 'uint32': '<u4', 'float': '<f4', 'float32': '<f4', 'double': '<f8',
              'float64': '<f8'}


def _ply_header(f, ply_path):
    """(format, vertex count, [(name, numpy type)] of `element vertex`) of the PLY open (binary) at its start; the file is left at
    the first byte after end_header.  ValueError for anything _load_ply cannot read."""
    fmt, n, props, element, ended = 'ascii', 0, [], None, False
    for k, raw in enumerate(iter(f.readline, b'')):
        line = raw.decode('ascii', errors='replace')
        tok = line.split()
        if k == 0 and tok[:1] != ['ply']:
            raise ValueError(f"{ply_path}: not a PLY file")
        if line.startswith('end_header'):
            ended = True
            break
        if not tok:
            continue
        if tok[0] == 'format':
            fmt = tok[1] if len(tok) > 1 else ''
            if fmt not in ('ascii', 'binary_little_endian') or (fmt != 'ascii' and tok[2:3] != ['1.0']):
                raise ValueError(f"{ply_path}: format {' '.join(tok[1:])!r} is not supported (ascii or binary_little_endian 1.0)")
        elif tok[0] == 'element':
            element = tok[1] if len(tok) > 1 else None
            if line.startswith('element vertex'):
                n = int(tok[-1])
        elif tok[0] == 'property' and element == 'vertex':
            if len(tok) > 1 and tok[1] == 'list':
                raise ValueError(f"{ply_path}: a list property on the vertex element is not supported")
            if len(tok) != 3 or tok[1] not in _PLY_TYPES:
                raise ValueError(f"{ply_path}: vertex property {' '.join(tok[1:])!r} has an unsupported type")
            props.append((tok[2], _PLY_TYPES[tok[1]]))
    if not ended:
        raise ValueError(f"{ply_path}: no end_header")
    return fmt, n, props


def _load_ply(ply_path):
    """A PLY's vertices, sanitised by _filter_points on x y z (data_loader.py:78-104 for ASCII; the header is read properly: `format
    ascii` or `binary_little_endian 1.0`, the property list of `element vertex` with the scalar types float / double / uchar and the
    int types; anything else, binary_big_endian or a list property on the vertex element: ValueError; other elements after the
    vertices are ignored).
      * ASCII: [N, 3], the first three numbers of each vertex line, exactly as the reference reads it -- the colour columns of an
        ASCII file are dropped, as they always were.
      * binary_little_endian (what COLMAP and the INRIA tools write): x y z by name, and when red, green and blue exist the result is
        [N, 6] with the colours in the file's own range (initialize_gaussians_from_pointcloud divides by 255 when the maximum
        exceeds 1), filtered with their rows."""
    with open(ply_path, 'rb') as f:
        fmt, n, props = _ply_header(f, ply_path)
        body = f.read()
    if fmt == 'ascii':
        pts = []
        lines = body.decode('utf-8', errors='replace').replace('\r\n', '\n').replace('\r', '\n').split('\n')
        for line in lines[:-1] if lines[-1] == '' else lines:       # (the lines a text-mode file object yields)
            if len(pts) < n:
                pts.append([float(v) for v in line.split()[:3]])
        return _filter_points(torch.tensor(pts, dtype=torch.float32).reshape(-1, 3))
    names = [name for name, _ in props]
    if len(set(names)) != len(names) or not all(k in names for k in 'xyz'):
        raise ValueError(f"{ply_path}: the vertex element needs one x, y and z property each (it has {names})")
    dtype = np.dtype(props)
    if len(body) < n * dtype.itemsize:
        raise ValueError(f"{ply_path}: {n} vertices of {dtype.itemsize} bytes announced, {len(body)} bytes present")
    v = np.frombuffer(body, dtype=dtype, count=n)

    def cols(keys):
        return torch.from_numpy(np.stack([v[k].astype(np.float32) for k in keys], axis=1)).reshape(-1, len(keys))

    has_rgb = all(k in names for k in ('red', 'green', 'blue'))
    return _filter_points(cols('xyz'), cols(('red', 'green', 'blue')) if has_rgb else None)


def load_point_cloud(pcd_path):
    """.ply (ASCII or binary little-endian: _load_ply) / .npy / .pt -> [N, 3+] float tensor (data_loader.py:50-76)."""
    ext = Path(pcd_path).suffix.lower()
    if ext == '.pt':
        return torch.load(pcd_path, weights_only=True)
    if ext == '.npy':
        return torch.from_numpy(np.load(pcd_path)).float()
    if ext == '.ply':
        return _load_ply(pcd_path)
    raise ValueError(f"Unsupported point cloud format: {ext}")


class GaussianDataset:
    """Images + intrinsics + camera-to-world poses in the reference layout (data_loader.py:153-284); same constructor
    arguments (scale_factor defaults to 0.5 there too) and the same sample dict.  Not in the reference (keyword-only, off by
    default): alpha=True adds sample['alpha'] [H, W], the file's alpha channel (1.0 for a file without one), rescaled bilinearly with
    the image; depth_dir='depth' adds sample['depth'] [H, W] from <data_dir>/<depth_dir>/<image stem>.npy (float32 camera-space z, <= 0
    or non-finite = no data), rescaled with mode='nearest' so that the zeros do not bleed into valid depths."""

    def __init__(self, data_dir, image_dir='images', cam_meta_path=None, scale_factor=0.5, *, alpha=False, depth_dir=None):
        self.alpha = bool(alpha)
        self.depth_dir = depth_dir
        self.data_dir = Path(data_dir)
        self.image_dir = self.data_dir / image_dir
        self.scale_factor = scale_factor
        self.cam_params = load_camera_parameters(self.data_dir / 'cam_meta.npy' if cam_meta_path is None else Path(cam_meta_path))
        self.image_files = sorted(f for ext in ('*.jpg', '*.png', '*.JPG', '*.PNG') for f in self.image_dir.glob(ext))
        if not self.image_files:
            raise ValueError(f"No images found in {self.image_dir}")
        self.c2w_matrices = self._load_camera_poses()

    def _load_camera_poses(self):
        pose_file = self.data_dir / 'poses.npy'
        if pose_file.exists():
            return [torch.from_numpy(p).float() for p in np.load(pose_file)]
        c2w = self.cam_params.get('c2w') if isinstance(self.cam_params, dict) else None
        if isinstance(c2w, (list, np.ndarray)):
            return [torch.from_numpy(np.asarray(p)).float() for p in c2w]
        return None

    def __len__(self):
        return len(self.image_files)

    def __getitem__(self, idx):
        extra = {}
        if self.alpha:
            image, extra['alpha'] = load_image_alpha(self.image_files[idx])
        else:
            image = load_image(self.image_files[idx])
        if self.depth_dir is not None:
            depth = torch.from_numpy(np.asarray(np.load(self.data_dir / self.depth_dir / (self.image_files[idx].stem + '.npy')), dtype=np.float32))
            if tuple(depth.shape) != tuple(image.shape[:2]):
                raise ValueError(f"depth map of {self.image_files[idx].name} is {tuple(depth.shape)}, the image {tuple(image.shape[:2])}")
            extra['depth'] = depth
        if self.scale_factor != 1.0:
            h, w = image.shape[:2]
            size = (int(h * self.scale_factor), int(w * self.scale_factor))
            image = torch.nn.functional.interpolate(image.permute(2, 0, 1).unsqueeze(0),
                                                    size=size,
                                                    mode='bilinear', align_corners=False).squeeze(0).permute(1, 2, 0)
            if 'alpha' in extra:
                extra['alpha'] = torch.nn.functional.interpolate(extra['alpha'][None, None], size=size, mode='bilinear', align_corners=False)[0, 0]
            if 'depth' in extra:
                extra['depth'] = torch.nn.functional.interpolate(extra['depth'][None, None], size=size, mode='nearest')[0, 0]
        H, W = image.shape[:2]
        c2w = self.c2w_matrices[idx] if self.c2w_matrices is not None else torch.eye(4, dtype=torch.float32)
        cp, s = self.cam_params, self.scale_factor
        has_c = 'cx' in cp and 'cy' in cp
        return {'image': image, 'c2w': c2w, 'fx': cp['fx'] * s, 'fy': cp['fy'] * s, 'cx': cp['cx'] * s if has_c else W / 2.0,
                'cy': cp['cy'] * s if has_c else H / 2.0, 'H': H, 'W': W, 'idx': idx, **extra}


def split_views(n, hold=8):
    """(train_indices, test_indices) of a dataset of n images (not in the reference, which trains on all of them): every hold-th image
    -- i % hold == 0 -- is a held-out test view, the Mip-NeRF 360 / INRIA `--eval` convention (hold = 8).  hold < 1: ValueError."""
    if type(n) is not int or n < 0:
        raise ValueError(f"n must be an integer >= 0, not {n!r}")
    if type(hold) is not int or hold < 1:
        raise ValueError(f"hold must be an integer >= 1, not {hold!r}")
    return [i for i in range(n) if i % hold], [i for i in range(n) if i % hold == 0]


def initialize_gaussians_from_pointcloud(points, num_sh_bands=3, *, scale_init="reference", init_scale=1.0, device=None):
    """One Gaussian per point: log-scale -2 +- 0.1, identity quaternion (0,0,0,1), opacity_raw 0.1, colours from columns
    3-5 (divided by 255 if > 1) or uniform random, zero higher-order SH (data_loader.py:287-367).  Only num_sh_bands >= 3
    gives the [N, 45] f_rest that evaluate_sh / the HIP path accept (as in the reference).

    Not in the reference (keyword-only; the default is the reference's rule, draw for draw): scale_init="knn" starts every Gaussian
    as the isotropic blob of the paper, scale_raw = log(init_scale sqrt(max(d2, 1e-7))) in all three columns with d2 the mean squared
    distance to the three nearest neighbours (knn.init_scale_raw; a HIP search, so the points must be on a GPU); every other field is
    as with "reference" under the same seed.  device: where the points are moved first and everything is returned (None: the points'
    own device; "knn" with CPU points and no device= is a RuntimeError)."""
    if scale_init not in ("reference", "knn"):
        raise ValueError(f"scale_init must be 'reference' or 'knn', not {scale_init!r}")
    if isinstance(init_scale, bool) or not isinstance(init_scale, (int, float)) or not 0.0 < init_scale < float("inf"):
        raise ValueError(f"init_scale must be a finite number > 0, not {init_scale!r}")
    if not isinstance(points, torch.Tensor):
        points = torch.from_numpy(np.asarray(points)).float()
    if device is not None:
        points = points.to(device)
    if scale_init == "knn" and not points.is_cuda:
        raise RuntimeError("scale_init='knn' runs on the GPU and there is no CPU fallback: pass device= (the points are on the CPU)")
    n, dev = points.shape[0], points.device
    pos = points[:, :3]
    scale_raw = torch.randn(n, 3, device=dev) * 0.1 - 2.0
    if scale_init == "knn":                                  # (after the draw: the colours below come out as with "reference")
        from . import knn
        scale_raw = knn.init_scale_raw(pos.to(torch.float32).contiguous(), float(init_scale))
    q_raw = torch.zeros(n, 4, device=dev)
    q_raw[:, 3] = 1.0
    opacity_raw = torch.ones(n, device=dev) * 0.1
    if points.shape[1] >= 6:
        colors = points[:, 3:6]
        if colors.max() > 1.0:
            colors = colors / 255.0
    else:
        colors = torch.rand(n, 3, device=dev)
    width = 45 if num_sh_bands >= 3 else (9 if num_sh_bands == 1 else 0)
    return {'pos': pos, 'opacity_raw': opacity_raw, 'f_dc': colors, 'f_rest': torch.zeros(n, width, device=dev),
            'scale_raw': scale_raw, 'q_raw': q_raw}


def write_dataset(data_dir, images, fx, fy, poses, points=None, cx=None, cy=None, alphas=None, depths=None):
    """Write a scene in the reference layout: images/000000.png ..., cam_meta.npy, poses.npy, pointcloud.ply (ASCII).  alphas (one
    [H, W] per image): the PNGs are RGBA; depths (one [H, W] per image): depth/000000.npy ... in float32 (GaussianDataset alpha=True,
    depth_dir='depth')."""
    from PIL import Image
    d = Path(data_dir)
    (d / 'images').mkdir(parents=True, exist_ok=True)

    def host(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    for i, im in enumerate(images):
        a = im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        if alphas is not None:
            a = np.concatenate([a[..., :3], host(alphas[i])[..., None]], axis=-1)
        Image.fromarray((np.clip(a, 0, 1) * 255).round().astype(np.uint8)).save(d / 'images' / f'{i:06d}.png')
    if depths is not None:
        (d / 'depth').mkdir(parents=True, exist_ok=True)
        for i, z in enumerate(depths):
            np.save(d / 'depth' / f'{i:06d}.npy', host(z).astype(np.float32))
    h, w = (images[0].shape[0], images[0].shape[1])
    meta = {'fx': float(fx), 'fy': float(fy), 'height': int(h), 'width': int(w)}
    if cx is not None and cy is not None:
        meta.update(cx=float(cx), cy=float(cy))
    np.save(d / 'cam_meta.npy', meta, allow_pickle=True)        # the reference's format (its loader needs the pickle)
    with open(d / 'cam_meta.json', 'w') as f:                     # same content, read in preference by load_camera_parameters
        json.dump(meta, f)
    np.save(d / 'poses.npy', np.asarray(poses, dtype=np.float32))
    if points is not None:
        p = np.asarray(points, dtype=np.float64)
        with open(d / 'pointcloud.ply', 'w') as f:
            f.write(f"ply\nformat ascii 1.0\nelement vertex {len(p)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
            for x, y, z in p[:, :3]:
                f.write(f"{x:.9g} {y:.9g} {z:.9g}\n")
