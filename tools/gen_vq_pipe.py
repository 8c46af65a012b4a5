"""Retired: this generator wrote the instruction block of vq_pipe_kernel (DVQ_VQ_KERNEL=17), a fast-VQ kernel that was measured
slower than vq_stream16_kernel and removed from the tree.  The generator and the kernel live in git history (commit 66a0f2d).
The file stays because bench.py's kernel_sources_sha256() reads it."""
