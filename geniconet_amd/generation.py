"""Shapes drawn from the variational autoencoder, and their score as a SET (metrics.generation_metrics): what a user of ico2ico_vae
needs to say how good its samples are -- a generated shape has no target, so none of the reconstruction figures applies.

    z = sample_prior(model, count, seed)                     latents, the same on every device
    v = generate_vertices(model, z, batch_size)              (count, V, 3) vertices of the decoded shapes
    evaluate_generation(model, reference_vertices, count)    dict(mmd=, cov=, one_nna=) against a set of reference shapes

The latents come from N(0, I), or with `misc` -- what train.train_epoch saves with every checkpoint of the VAE losses, the mu and
logvar of the epoch's last training batch -- from trn_mean + trn_logvar eps, exactly the formula of models.enc2ico_vae.createSample
(the reference's: logvar itself scales eps, not exp(logvar / 2)).  eps is always drawn on the CPU, from a generator seeded with `seed`.
"""
import torch

from . import geometry, metrics, models


def latent_shape(model):
    """(C, H, W) of one latent of `model` (ico2ico_vae, enc2ico_vae): what model.mu produces for the model's own input size -- a
    stride-2 convolution at level subdivisions - 2, so the grid of level r = subdivisions - 3, (5 2^r, 2^(r + 1))."""
    r = model.subdivisions - 3
    if r < 0:
        raise ValueError('generation: the model needs subdivisions >= 3, got %d' % model.subdivisions)
    mu = getattr(model, 'mu', None)
    channels = mu[0].out_features if mu is not None else models.VAE_LATENT_CHANNELS
    return channels, 5 * 2 ** r, 2 ** (r + 1)


def _device_of(model):
    return next(model.parameters()).device


def _count(who, name, value):
    if isinstance(value, bool) or not isinstance(value, int) or value < 1:
        raise ValueError('%s: %s must be a positive integer, got %r' % (who, name, value))
    return value


def sample_prior(model, count, seed=0, misc=None):
    """`count` latents (count, C, H, W) fp32 of latent_shape(model), on the model's device.  eps = torch.randn((count, C, H, W),
    generator=g), g a CPU generator seeded with `seed`: the same latents on every device.  Without `misc` the latents are eps, a draw
    from the prior N(0, I).  With misc -- a dict with 'trn_mean' and 'trn_logvar' of shape (B, C, H, W), or the list holding it that
    createSample takes -- latent k is trn_mean[k mod B] + trn_logvar[k mod B] * eps[k]: for count = B, createSample's formula."""
    who = 'sample_prior'
    _count(who, 'count', count)
    shape = latent_shape(model)
    eps = torch.randn((count,) + shape, generator=torch.Generator().manual_seed(seed))
    if misc is not None:
        if isinstance(misc, (list, tuple)):
            misc = misc[0]
        mean, logvar = misc['trn_mean'].detach().cpu().float(), misc['trn_logvar'].detach().cpu().float()
        if mean.dim() != 4 or mean.shape != logvar.shape or tuple(mean.shape[1:]) != shape or mean.shape[0] < 1:
            raise ValueError('%s: trn_mean and trn_logvar must both be (B,) + %s, got %s and %s'
                             % (who, shape, tuple(mean.shape), tuple(logvar.shape)))
        rows = torch.arange(count) % mean.shape[0]
        eps = torch.add(mean[rows], logvar[rows] * eps)
    return eps.to(_device_of(model))


def generate_vertices(model, latents, batch_size=16):
    """(count, V, 3) vertices of the shapes model.decode makes of `latents` (count, C, H, W), `batch_size` at a time: the decoder in
    eval mode (the running statistics of its BatchNorms, as at test time) and without a graph, its output grid through
    metrics.output2vertices (the two poles appended).  The model's training flag is put back."""
    who = 'generate_vertices'
    _count(who, 'batch_size', batch_size)
    if not torch.is_tensor(latents) or latents.dim() != 4 or latents.shape[0] < 1 or tuple(latents.shape[1:]) != latent_shape(model):
        raise ValueError('%s: expected latents (count,) + %s, got %s'
                         % (who, latent_shape(model), tuple(latents.shape) if torch.is_tensor(latents) else type(latents).__name__))
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            z = latents.to(_device_of(model))
            return torch.cat([metrics.output2vertices(model.subdivisions, model.decode(z[lo:lo + batch_size]))
                              for lo in range(0, z.shape[0], batch_size)])
    finally:
        model.train(was_training)


def evaluate_generation(model, reference_vertices, count, seed=0, samples=0, faces=None, misc=None, batch_size=16, distance='chamfer', points=0, jsd=0):
    """dict(mmd=, cov=, one_nna=) of Python floats (metrics.generation_metrics): `count` shapes drawn from the model (sample_prior with
    `seed` and `misc`, generate_vertices) against the reference shapes reference_vertices (R, V, 3).  The point sets are the vertices,
    or with samples = S > 0 metrics' convention for surface samples: sampling.sample_points of both sets of surfaces over `faces`
    (F, 3; default the icosahedral grid's own, geometry.get_ico_faces) from uniforms torch.rand((2, S, 3), generator=g), g a CPU
    generator seeded with `seed` -- every generated surface takes the first S, every reference surface the second: the same samples on
    every device.  distance: 'chamfer' (default) or 'emd', as in metrics.generation_metrics.  points = P > 0 thins every point set to
    its P farthest points (sampling.farthest_points) after the optional surface sampling, so samples=S, points=P is "S surface samples
    thinned to P", as in metrics.generation_metrics; points=0 (default) keeps them whole.  jsd = R > 0 adds the key 'jsd', the
    Jensen-Shannon divergence of the occupancy distributions of the two sets on a lattice of R lattice points an axis over (-1, 1)
    (metrics.jensen_shannon_divergence; 28 in the shape-generation tables, at most 32), on exactly the point sets the matrices see --
    after samples= and points=; the lattice is the whole cube, not the lattice points inside the inscribed sphere that some code
    bases keep.  jsd=0 (default) returns the three keys alone."""
    who = 'evaluate_generation'
    if distance not in metrics.GENERATION_DISTANCES:
        raise ValueError('%s: distance must be one of %s, got %r' % (who, metrics.GENERATION_DISTANCES, distance))
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 0:
        raise ValueError('%s: samples must be a non-negative integer, got %r' % (who, samples))
    metrics._check_subset_size(who, points)
    metrics._check_jsd_resolution(who, jsd)
    if not torch.is_tensor(reference_vertices) or reference_vertices.dim() != 3 or reference_vertices.shape[-1] != 3:
        raise ValueError('%s: expected reference_vertices (R, V, 3), got %s'
                         % (who, tuple(reference_vertices.shape) if torch.is_tensor(reference_vertices) else type(reference_vertices).__name__))
    generated = generate_vertices(model, sample_prior(model, count, seed, misc), batch_size)
    reference = reference_vertices.detach().to(device=generated.device, dtype=generated.dtype)
    if samples:
        from .sampling import sample_points
        if faces is None:
            faces = torch.from_numpy(geometry.get_ico_faces(model.subdivisions))
        u = torch.rand((2, samples, 3), generator=torch.Generator().manual_seed(seed)).to(device=generated.device, dtype=generated.dtype)
        with torch.no_grad():
            generated = sample_points(generated, faces, uniforms=u[0].expand(generated.shape[0], -1, -1))[0]
            reference = sample_points(reference, faces, uniforms=u[1].expand(reference.shape[0], -1, -1))[0]
    return metrics.generation_metrics(generated, reference, distance, points, jsd)
