"""The ctypes bindings of the geometry kernels, one module per kernel file of csrc/ (triangulation.py binds geometry.hip).
The public spelling of every name here is geometry.<name>; the argument idioms the wrappers share are in _args.py."""
