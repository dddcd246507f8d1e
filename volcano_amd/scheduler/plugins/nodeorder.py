"""Nodeorder plugin (reference ``plugins/nodeorder/nodeorder.go:34-66``).

Weighted sum of leastrequested / mostrequested / balancedallocation — the
three analytic terms of the fused score kernel (K2).  Taint-toleration and
affinity hard filters are handled by the predicates plugin's bit planes;
a soft topology-spread entry (``whenUnsatisfiable: ScheduleAnyway``) is
scored per placement by the topologyspread plugin's own select
(``exact: true`` there), not here.

The select scores a class once and fills nodes in that order; the reference
scores per task, so a node that just took a pod scores lower (or higher) for
the next one.  With the plugin argument ``exact: true`` the plugin publishes
``ssn.score_exact`` and the allocate action has every class of two or more
instances re-score its chosen node after each placement, on the device
(``rescore_select``): three replicas over three empty twin nodes land one
each under ``leastrequested``, where the static fill puts all three on node
0.  It only changes a decision where ``leastrequested.weight`` or
``balancedresource.weight`` is nonzero, so only then is a class flagged;
classes under a topology-spread rule keep their own select, and the flag is
ignored under the soft-shard coordinator, like every exact rule.
"""

from __future__ import annotations

from .base import Plugin, register


@register("nodeorder")
class NodeOrderPlugin(Plugin):
    def on_session_open(self, ssn) -> None:
        ssn.score_weights["least"] = float(
            self.args.get("leastrequested.weight", 1.0))
        ssn.score_weights["bal"] = float(
            self.args.get("balancedresource.weight", 1.0))
        most = float(self.args.get("mostrequested.weight", 0.0))
        if most:
            ssn.score_weights["most"] = ssn.score_weights.get("most", 0.0) + most
        if str(self.args.get("exact", False)).lower() in ("1", "true", "yes"):
            ssn.score_exact = True
