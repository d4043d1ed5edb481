"""The binding layer below ``egtr_amd.ops``: one thin Python function per C entry of libegtr_hip.so, grouped the way csrc/ is
grouped.  Nothing in this package reads a route switch or imports ``ops``; ``ops`` star-imports every module here and stays
the public namespace.  Modules: ``backbone``, ``derived``, ``elementwise``, ``heads``, ``linear``, ``protocols`` (the PredCls /
SGCls candidate builder, csrc/matched_topk.hip), ``statistics``, ``vrd``."""
