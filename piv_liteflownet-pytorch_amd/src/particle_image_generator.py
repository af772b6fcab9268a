"""Alias of pivlfn.particles under the reference's import path (src/particle_image_generator.py): ParticleImageGen with the
reference's constructor and method names, seeding on the host, moving and drawing the particles on the GPU."""
from pivlfn.particles import (BAD, LOST, PairParticles, ParticleImageGen, ParticleImages, displace_particles,  # noqa: F401
                              render_particles)
